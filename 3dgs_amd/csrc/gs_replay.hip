// gs_replay.hip -- the kernels that walk a recorded forward again (gs_render.h: ReplayArgs), for gfx950:
//   contributions_kernel   per-gaussian blend-weight statistics          (gsplat_context_accumulate_contributions)
//   median_depth_kernel    z of the entry at which T falls to a threshold (gsplat_context_median_depth)
//   features_fwd_kernel    out[p, c]     = sum_i w_ip f[g_i, c]          (gsplat_context_render_features)
//   features_lift_kernel   lifted[g, c] += sum_p w_gp map[p, c]          (gsplat_context_lift_features)
//   features_bwd_kernel    the map's gradient with respect to the geometry (gsplat_context_features_backward)
// with w_ip = alpha * T(before) of entry i of the tile's list at pixel p, over the entries the forward composited: i < n(p),
// the forward's stop index, and alpha past the forward's 1/255 test.
// The walk, common to all four: one workgroup per tile, lanes on pixels and batches of staged records as in
// render_fwd_kernel -- the same load_record / block_hits / stage_record / row lists, so the same (gaussian, block) pairs
// are visited and alpha and T come out bit for bit (T exactly for a list the forward walked whole; a segmented forward
// multiplied its segments' products in another order).  block_hits is recomputed as the forward does: a render-only
// forward stores no masks.  A row builds no list beyond its own largest stop index, the workgroup leaves at the tile's.
// A list longer than kSegSplitMin is walked whole by the one workgroup (correct, and as slow as the unsegmented forward
// was on such lists).  Outside pixels of partial tiles carry T = 0 and n = 0, read and write nothing.
// The feature kernels take the caller's channels f[N,C] (global order) in chunks of K = 4, 8 or 16 (one K per launch: the
// smallest that holds C, 16 beyond); gridDim.y counts the chunks, every chunk walks the tile's list again.  No
// background term on either side of render / lift (the caller has T), nothing of the geometry is differentiated there.
#include "gs_common.h"
#include "gs_launch.h"
#include "gs_render.h"

namespace gs {

__host__ __device__ inline int tiles_x(const ReplayArgs &a) { return (a.width + 15) / 16; }
__host__ __device__ inline int tile_count(const ReplayArgs &a) { return tiles_x(a) * ((a.height + 15) / 16); }

// ---- the walk's blocks ----------------------------------------------------------------------------------------------
// A thread's place in the workgroup -- every 16-lane row of a wave owns one 4x4 pixel block, one pixel per lane -- and
// what it needs of its tile and pixel.
struct TilePixel {
  int wave, lane, row, j;
  int pid;           // py * width + px; valid when `inside`
  bool inside;       // the pixel lies in the image
  float fpx, fpy;    // the pixel
  float tx0, ty0;    // the tile's first pixel
  int start;         // the tile's list is sorted[start ..]
  int n;             // the pixel's stop index, at most the list's length; 0 outside the image
};
__device__ __forceinline__ TilePixel tile_pixel(const ReplayArgs &a, int tile) {
  TilePixel p;
  const int tid = threadIdx.x, ntx = tiles_x(a);
  p.wave = tid >> 6; p.lane = tid & 63; p.row = p.lane >> 4; p.j = p.lane & 15;
  const int tile_x = tile % ntx, tile_y = tile / ntx;
  const int px = tile_x * 16 + (p.wave & 1) * 8 + (p.row & 1) * 4 + (p.j & 3);
  const int py = tile_y * 16 + (p.wave >> 1) * 8 + (p.row >> 1) * 4 + (p.j >> 2);
  p.inside = px < a.width && py < a.height;
  p.pid = py * a.width + px;
  p.fpx = (float)px; p.fpy = (float)py;
  p.tx0 = (float)(tile_x * 16); p.ty0 = (float)(tile_y * 16);
  p.start = a.ranges[tile];
  const int total = a.ranges[tile + 1] - p.start;
  p.n = p.inside ? min(a.n_px[p.pid], total) : 0;
  return p;
}

// the all-zero sentinel record behind a batch of kB slots, and the cleared cell the tile's top is merged in
template <int kB>
__device__ __forceinline__ void walk_setup(float4 *s_r0, float4 *s_r1, int *s_tile_top) {
  if (threadIdx.x == 0) {
    s_r0[kB] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    s_r1[kB] = sentinel_r1();
    *s_tile_top = 0;
  }
}

// The largest stop index of each of the wave's four rows and of the wave (wave-uniform).  The tile's is their maximum
// over the four waves: each kernel merges `wave` into its cleared LDS cell between two barriers and reads `tile` back.
struct WalkTops { int row0, row1, row2, row3, wave, tile; };
__device__ __forceinline__ WalkTops walk_tops(int n) {
  WalkTops t;
  const int row_top = row_max_int(n);
  t.row0 = __builtin_amdgcn_readlane(row_top, 0); t.row1 = __builtin_amdgcn_readlane(row_top, 16);
  t.row2 = __builtin_amdgcn_readlane(row_top, 32); t.row3 = __builtin_amdgcn_readlane(row_top, 48);
  t.wave = max(max(t.row0, t.row1), max(t.row2, t.row3));
  t.tile = 0;
  return t;
}

// the wave's four row lists ([wave][row][kStride] in s_list) of the staged batch that starts at entry `base`, none beyond a
// row's top; returns the trips
template <int kStride>
__device__ __forceinline__ int walk_lists(const float4 *s_r1, unsigned short *s_list, int count, const TilePixel &p,
                                          const WalkTops &t, int base) {
  const RowCounts rc = build_row_lists<kStride>(s_r1, s_list + p.wave * 4 * kStride, count, p.wave, p.lane, t.row0 - base,
                                                t.row1 - base, t.row2 - base, t.row3 - base, 1);
  return max(max(rc.c0, rc.c1), max(rc.c2, rc.c3));
}

// Entry `entry` of the tile's list as the loops evaluate it, with its block-hit bits; returns the gaussian's compact id.
__device__ __forceinline__ int staged_entry(const ReplayArgs &a, const TilePixel &p, int entry, SplatRec &s,
                                            unsigned int &hits) {
  const RawSplats none = {nullptr, nullptr, nullptr, nullptr};
  const int g = a.sorted[p.start + entry];
  s = load_record<true>(g, a.recs, none);
  hits = block_hits(s, p.tx0, p.ty0);
  stage_record(s);
  return g;
}
// ... parked in `slot` for the front-to-back trips: r0 = (u, v, a2, b2), r1 = (c2, log2 opa, the exponent's bound
// min(log2 opa, log2 0.99) as render_fwd_kernel forms it, block-hit bits)
__device__ __forceinline__ int stage_capped(const ReplayArgs &a, const TilePixel &p, int entry, float4 *s_r0, float4 *s_r1,
                                            int slot) {
  SplatRec s;
  unsigned int hits;
  const int g = staged_entry(a, p, entry, s, hits);
  s_r0[slot] = s.r0;
  s_r1[slot] = make_float4(s.r1.x, s.r1.y, s.r1.y > kLog2AlphaMax ? kLog2AlphaMax : s.r1.y, __uint_as_float(hits));
  return g;
}

// One front-to-back trip: the pixel's blend weight alpha * T(before) of the staged record at byte offset `off` of the
// batch that starts at entry `base`, and T moved behind it.  `on`: the forward composited the entry at this pixel; the
// weight is 0 otherwise.  A row past the end of its list reads the sentinel record: alpha 0.
__device__ __forceinline__ float trip_weight(const float4 *s_r0, const float4 *s_r1, int off, int base, const TilePixel &p,
                                             float &T, bool &on) {
  const float4 a = *reinterpret_cast<const float4 *>(reinterpret_cast<const char *>(s_r0) + off);
  const float4 b = *reinterpret_cast<const float4 *>(reinterpret_cast<const char *>(s_r1) + off);
  float al = staged_alpha_capped(a.z, a.w, b.x, b.y, b.z, a.x - p.fpx, a.y - p.fpy);
  on = al > kAlphaMin && base + (off >> 4) < p.n;
  al = on ? al : 0.0f;
  const float w = al * T;
  T = __builtin_fmaf(-al, T, T);
  return w;
}

// The chunk's slice [c0, c0 + K) of the feature rows of the `count` list entries from sorted[first] into s_feat[slot][K],
// zeros beyond C: (slot, channel) spread over all 256 threads, so the K channels of a row are one coalesced read; every
// thread finds its row through sorted and compact_to_global itself, which keeps the gather in front of the batch's one
// staging barrier.
template <int K>
__device__ __forceinline__ void gather_features(const ReplayArgs &a, int first, int count, int c0, int channels,
                                                const float *__restrict__ features, float *s_feat) {
  for (int e = threadIdx.x; e < count * K; e += 256) {  // (slot, channel) = (e / K, e % K)
    const int c = c0 + (e & (K - 1));
    const size_t gi = (size_t)a.c2g[a.sorted[first + e / K]];
    s_feat[e] = c < channels ? features[gi * (size_t)channels + c] : 0.0f;
  }
}

// The pixel's channels [c0, c0 + K) of a caller's [H,W,C] array; an outside pixel and the channels beyond C: zeros.
// vec (with_chunks): whole 16-byte accesses.
template <int K>
__device__ __forceinline__ void load_chunk(const float *__restrict__ array, const TilePixel &p, int c0, int channels, int vec,
                                           float (&m)[K]) {
#pragma unroll
  for (int c = 0; c < K; ++c) m[c] = 0.0f;
  if (!p.inside) return;
  const float *src = array + (size_t)p.pid * (size_t)channels + c0;
  if (vec) {
#pragma unroll
    for (int q = 0; q < K / 4; ++q)
      if (c0 + 4 * q < channels) {
        const float4 v = reinterpret_cast<const float4 *>(src)[q];
        m[4 * q] = v.x; m[4 * q + 1] = v.y; m[4 * q + 2] = v.z; m[4 * q + 3] = v.w;
      }
  } else {
#pragma unroll
    for (int c = 0; c < K; ++c)
      if (c0 + c < channels) m[c] = src[c];
  }
}
template <int K>
__device__ __forceinline__ void store_chunk(float *__restrict__ array, const TilePixel &p, int c0, int channels, int vec,
                                            const float (&m)[K]) {
  if (!p.inside) return;
  float *dst = array + (size_t)p.pid * (size_t)channels + c0;
  if (vec) {
#pragma unroll
    for (int q = 0; q < K / 4; ++q)
      if (c0 + 4 * q < channels) reinterpret_cast<float4 *>(dst)[q] = make_float4(m[4 * q], m[4 * q + 1], m[4 * q + 2], m[4 * q + 3]);
  } else {
#pragma unroll
    for (int c = 0; c < K; ++c)
      if (c0 + c < channels) dst[c] = m[c];
  }
}

// ---- contributions: the walk reduced per gaussian instead of per pixel.  Per trip every 16-lane row holds one
// (gaussian, 4x4 block) pair: the row's sum (row_sum), maximum (row_max_int on the bit pattern: weights are >= 0) and
// pixel count (the row's 16 bits of the ballot) go from the row's first lane into the batch's three LDS accumulators (the
// four rows of a wave are on four different gaussians, so the LDS atomic IS the step across the wave and across the four
// waves), and behind the batch thread t < count sends slot t's totals to the caller's arrays at compact_to_global: one
// global atomic per statistic and (tile, gaussian), none when no pixel of the tile composited the gaussian.  The sum is a
// float atomic (order-dependent in its last bits); the maximum and the count are exact whatever the order.
__global__ __launch_bounds__(256) void contributions_kernel(ReplayArgs a, float *__restrict__ weight_sum,
                                                            unsigned int *__restrict__ weight_max, int *__restrict__ pixels) {
  __shared__ float4 s_r0[kBatch + 1], s_r1[kBatch + 1];  // stage_capped's; [kBatch]: the sentinel
  __shared__ float s_sum[kBatch + 1];
  __shared__ int s_max[kBatch + 1], s_cnt[kBatch + 1], s_gid[kBatch];
  __shared__ int s_tile_top;
  __shared__ __attribute__((aligned(16))) unsigned short s_list[16 * kListStride + 2];
  const int tile = ordered_tile(nullptr, (int)blockIdx.x, tile_count(a));
  if (tile >= tile_count(a)) return;
  const int tid = threadIdx.x;
  walk_setup<kBatch>(s_r0, s_r1, &s_tile_top);
  const TilePixel p = tile_pixel(a, tile);
  WalkTops tops = walk_tops(p.n);
  __syncthreads();
  if (p.lane == 0) atomicMax(&s_tile_top, tops.wave);
  __syncthreads();
  tops.tile = s_tile_top;
  const unsigned short *my_list = s_list + (p.wave * 4 + p.row) * kListStride;  // this row's of the wave's four lists
  float T = p.inside ? 1.0f : 0.0f;
  for (int base = 0; base < tops.tile; base += kBatch) {
    const int count = min(kBatch, tops.tile - base);
    __syncthreads();  // the flush of the batch before has read the accumulators
    if (tid < count) s_gid[tid] = stage_capped(a, p, base + tid, s_r0, s_r1, tid);
    if (tid <= kBatch) { s_sum[tid] = 0.0f; s_max[tid] = 0; s_cnt[tid] = 0; }
    __syncthreads();
    const int trips = walk_lists<kListStride>(s_r1, s_list, count, p, tops, base);
    for (int i = 0; i < trips; ++i) {
      const int off = my_list[i];
      bool on;
      const float w = trip_weight(s_r0, s_r1, off, base, p, T, on);
      const float sum = row_sum(w);
      const int top_w = row_max_int(__float_as_int(w));
      const int cnt = __popc((unsigned int)(__ballot(on) >> (p.row * 16)) & 0xFFFFu);
      if (p.j == 0 && cnt > 0) {
        const int slot = off >> 4;
        atomicAdd(&s_sum[slot], sum);
        atomicMax(&s_max[slot], top_w);
        atomicAdd(&s_cnt[slot], cnt);
      }
    }
    __syncthreads();
    if (tid < count) {
      const int cnt = s_cnt[tid];
      if (cnt > 0) {
        const int gi = a.c2g[s_gid[tid]];
        if (weight_sum) atomicAdd(weight_sum + gi, s_sum[tid]);
        if (weight_max) atomicMax(weight_max + gi, (unsigned int)s_max[tid]);
        if (pixels) atomicAdd(pixels + gi, cnt);
      }
    }
  }
}

// ---- median depth: the walk reduced to the first entry behind which the pixel's transmittance has fallen to
// `threshold`.  z of the batch's gaussians (the compacted xyz_c, as the forward stored it) is staged beside the records in
// s_z; a lane keeps T, the answer and its list position, and an answer once found is never replaced: no atomics, nothing
// written but the two maps, the same bits in every run and under either binning route.  A pixel is done when it has its
// answer or the batch starts at or behind its stop index; a wave whose pixels are all done builds no lists, and the
// workgroup leaves at the batch's barrier when every pixel is (__syncthreads_and: one decision for the workgroup) -- a
// done pixel's state cannot change, so the exits change no bit.
__global__ __launch_bounds__(256) void median_depth_kernel(ReplayArgs a, const float *__restrict__ xyz_c, float threshold,
                                                           float *__restrict__ depth, int *__restrict__ index) {
  __shared__ float4 s_r0[kBatch + 1], s_r1[kBatch + 1];  // stage_capped's; [kBatch]: the sentinel
  __shared__ float s_z[kBatch + 1];
  __shared__ int s_tile_top;
  __shared__ __attribute__((aligned(16))) unsigned short s_list[16 * kListStride + 2];
  const int tile = ordered_tile(nullptr, (int)blockIdx.x, tile_count(a));
  if (tile >= tile_count(a)) return;
  const int tid = threadIdx.x;
  walk_setup<kBatch>(s_r0, s_r1, &s_tile_top);
  if (tid == 0) s_z[kBatch] = 0.0f;
  const TilePixel p = tile_pixel(a, tile);
  WalkTops tops = walk_tops(p.n);
  __syncthreads();
  if (p.lane == 0) atomicMax(&s_tile_top, tops.wave);
  __syncthreads();
  tops.tile = s_tile_top;
  const unsigned short *my_list = s_list + (p.wave * 4 + p.row) * kListStride;  // this row's of the wave's four lists
  float T = p.inside ? 1.0f : 0.0f;
  float z = 0.0f;
  int found = -1;
  for (int base = 0; base < tops.tile; base += kBatch) {
    const int count = min(kBatch, tops.tile - base);
    const bool done = found >= 0 || base >= p.n;
    // (also: the trips of the batch before have read the records and s_z)
    if (__syncthreads_and(done ? 1 : 0)) break;
    if (tid < count) {
      const int g = stage_capped(a, p, base + tid, s_r0, s_r1, tid);
      s_z[tid] = xyz_c[3 * (size_t)g + 2];
    }
    __syncthreads();
    if (__ballot(!done) == 0ull) continue;
    const int trips = walk_lists<kListStride>(s_r1, s_list, count, p, tops, base);
    for (int i = 0; i < trips; ++i) {
      const int off = my_list[i];
      bool on;
      (void)trip_weight(s_r0, s_r1, off, base, p, T, on);
      if (on && found < 0 && T <= threshold) {
        found = base + (off >> 4);
        z = s_z[off >> 4];
      }
    }
  }
  if (p.inside) {
    depth[p.pid] = z;
    if (index) index[p.pid] = found;
  }
}

// ---- features forward: per batch, beside the records, the chunk's slice of the batch's feature rows goes to LDS
// (gather_features), and per trip a lane does acc[c] = fma(w, s_feat[slot][c], acc[c]) on K/4 16-byte reads (the 16 lanes
// of a row read one address: a broadcast).  A pixel's sum runs in list order, one chain per channel, without atomics: the
// map carries the same bits in every run, under either binning route, at every C and after every kind of forward whose
// list was walked whole -- channel c of the forward's own colours IS the forward's image at background 0.
template <int K>
__global__ __launch_bounds__(256) void features_fwd_kernel(ReplayArgs a, int channels, const float *__restrict__ features,
                                                           float *__restrict__ out, int vec) {
  static_assert(K == 4 || K == 8 || K == 16, "chunk widths");
  constexpr int kQ = K / 4;  // 16-byte reads per feature row
  __shared__ float4 s_r0[kBatch + 1], s_r1[kBatch + 1];  // stage_capped's; [kBatch]: the sentinel
  __shared__ float4 s_feat[(kBatch + 1) * kQ];           // [slot][K]; the sentinel's row is zeros
  __shared__ int s_tile_top;
  __shared__ __attribute__((aligned(16))) unsigned short s_list[16 * kListStride + 2];
  const int tile = ordered_tile(nullptr, (int)blockIdx.x, tile_count(a));
  if (tile >= tile_count(a)) return;
  const int c0 = (int)blockIdx.y * K;  // (more than one chunk: K = 16)
  const int tid = threadIdx.x;
  walk_setup<kBatch>(s_r0, s_r1, &s_tile_top);
  if (tid < kQ) s_feat[kBatch * kQ + tid] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
  const TilePixel p = tile_pixel(a, tile);
  WalkTops tops = walk_tops(p.n);
  __syncthreads();
  if (p.lane == 0) atomicMax(&s_tile_top, tops.wave);
  __syncthreads();
  tops.tile = s_tile_top;
  const char *fb = reinterpret_cast<const char *>(s_feat);
  const unsigned short *my_list = s_list + (p.wave * 4 + p.row) * kListStride;  // this row's of the wave's four lists
  float T = p.inside ? 1.0f : 0.0f;
  float acc[K] = {};
  for (int base = 0; base < tops.tile; base += kBatch) {
    const int count = min(kBatch, tops.tile - base);
    __syncthreads();  // the trips of the batch before have read the records and the feature rows
    if (tid < count) stage_capped(a, p, base + tid, s_r0, s_r1, tid);
    gather_features<K>(a, p.start + base, count, c0, channels, features, reinterpret_cast<float *>(s_feat));
    __syncthreads();
    const int trips = walk_lists<kListStride>(s_r1, s_list, count, p, tops, base);
    for (int i = 0; i < trips; ++i) {
      const int off = my_list[i];  // (the sentinel's feature row: zeros)
      bool on;
      const float w = trip_weight(s_r0, s_r1, off, base, p, T, on);
      const float4 *f = reinterpret_cast<const float4 *>(fb + off * kQ);
#pragma unroll
      for (int q = 0; q < kQ; ++q) {
        const float4 v = f[q];
        acc[4 * q + 0] = __builtin_fmaf(w, v.x, acc[4 * q + 0]);
        acc[4 * q + 1] = __builtin_fmaf(w, v.y, acc[4 * q + 1]);
        acc[4 * q + 2] = __builtin_fmaf(w, v.z, acc[4 * q + 2]);
        acc[4 * q + 3] = __builtin_fmaf(w, v.w, acc[4 * q + 3]);
      }
    }
  }
  store_chunk<K>(out, p, c0, channels, vec, acc);
}

// ---- lift: the lane holds its pixel's K map values.  Per trip the row's 16 x K products w map[p, c] are reduced over
// the row by a transposed butterfly on DPP (row_transpose_sum: 47 VALU at K = 16, the products included, against 80 for K
// products and K row_sums) that leaves lane j with channel j's row total, so ONE ds_add_f64 per wave and trip adds all K
// totals of the four rows' (gaussian, block) pairs into the batch's LDS accumulators [slot][K]; behind the batch thread
// (slot, c) sends every non-zero total to lifted[compact_to_global[id], c]: one global float atomic per (tile, gaussian,
// channel), none for a gaussian no pixel of the tile composited.  Float atomics in arrival order: the lifted sums are
// order-dependent in their last bits, as the gradient rows and weight_sum are.
//
// The row's sums of w m[c], c < K, over its 16 lanes: lane j < K of every 16-lane row ends with channel j's.  Two folding
// stages inside the quad (lanes 1 and 2 apart: each keeps the half of the values its lane bit selects and takes the
// partner's partial of the same half, so lane (b1 b0) of a quad ends with the quad's sums of channels 4 i + 2 b1 + b0), two
// row rotations (by 8 and by 4 lanes: both keep a lane's place in its quad) that add the four quads, and a select of
// i = the lane's quad.  The first stage selects among the lane's own m, which no trip changes: the caller makes those
// selects once (transpose_operands: mk = what the lane keeps, ms = what it sends) and the products are formed on the
// selected halves.
template <int K>
__device__ __forceinline__ void transpose_operands(const float (&m)[K], int j, float (&mk)[K / 2], float (&ms)[K / 2]) {
  const bool b0 = (j & 1) != 0;
#pragma unroll
  for (int i = 0; i < K / 2; ++i) {
    mk[i] = b0 ? m[2 * i + 1] : m[2 * i];
    ms[i] = b0 ? m[2 * i] : m[2 * i + 1];
  }
}
template <int K>
__device__ __forceinline__ float row_transpose_sum(float w, const float (&mk)[K / 2], const float (&ms)[K / 2], int j) {
  const bool b1 = (j & 2) != 0;
  float u[K / 2], t[K / 4];
#pragma unroll
  for (int i = 0; i < K / 2; ++i) u[i] = w * mk[i] + dpp_take<0xB1>(w * ms[i]);  // quad_perm [1,0,3,2]
#pragma unroll
  for (int i = 0; i < K / 4; ++i) {
    const float keep = b1 ? u[2 * i + 1] : u[2 * i], send = b1 ? u[2 * i] : u[2 * i + 1];
    t[i] = keep + dpp_take<0x4E>(send);  // quad_perm [2,3,0,1]
    t[i] = dpp_add<0x128>(t[i]);         // row_ror:8
    t[i] = dpp_add<0x124>(t[i]);         // row_ror:4
  }
  float r = t[0];
  if constexpr (K >= 8) r = (j >> 2) == 1 ? t[1] : r;
  if constexpr (K >= 16) { r = (j >> 2) == 2 ? t[2] : r; r = (j >> 2) == 3 ? t[3] : r; }
  return r;
}

template <int K>
__global__ __launch_bounds__(256) void features_lift_kernel(ReplayArgs a, int channels, const float *__restrict__ map,
                                                            float *__restrict__ lifted, int vec) {
  static_assert(K == 4 || K == 8 || K == 16, "chunk widths");
  __shared__ float4 s_r0[kBatch + 1], s_r1[kBatch + 1];  // stage_capped's; [kBatch]: the sentinel
  // [slot][K]: the batch's totals; slot kBatch: the sentinel's (rows past the end of their list add zeros there).  Doubles
  // for the rate of the LDS atomic, as in render_bwd_kernel: ds_add_f32 retires about one lane every three cycles, and
  // with K lanes of each of a wave's four rows adding in every trip that bounded the kernel (K = 16 at 1080p: 1.22 ms
  // against 0.29 ms for contributions_kernel's walk); ds_add_f64 runs at LDS rate (profiles/microbench/lds_atomic_rate)
  __shared__ double s_acc[(kBatch + 1) * K];
  __shared__ int s_gid[kBatch];
  __shared__ int s_tile_top;
  __shared__ __attribute__((aligned(16))) unsigned short s_list[16 * kListStride + 2];
  const int tile = ordered_tile(nullptr, (int)blockIdx.x, tile_count(a));
  if (tile >= tile_count(a)) return;
  const int c0 = (int)blockIdx.y * K;  // (more than one chunk: K = 16)
  const int tid = threadIdx.x;
  walk_setup<kBatch>(s_r0, s_r1, &s_tile_top);
  const TilePixel p = tile_pixel(a, tile);
  float m[K], mk[K / 2], ms[K / 2];  // the pixel's map values of this chunk, and as the row reduction's first stage takes them
  load_chunk<K>(map, p, c0, channels, vec, m);
  transpose_operands<K>(m, p.j, mk, ms);
  WalkTops tops = walk_tops(p.n);
  __syncthreads();
  if (p.lane == 0) atomicMax(&s_tile_top, tops.wave);
  __syncthreads();
  tops.tile = s_tile_top;
  const unsigned short *my_list = s_list + (p.wave * 4 + p.row) * kListStride;  // this row's of the wave's four lists
  float T = p.inside ? 1.0f : 0.0f;
  for (int base = 0; base < tops.tile; base += kBatch) {
    const int count = min(kBatch, tops.tile - base);
    __syncthreads();  // the flush of the batch before has read the accumulators
    if (tid < count) s_gid[tid] = stage_capped(a, p, base + tid, s_r0, s_r1, tid);
    for (int e = tid; e < count * K; e += 256) s_acc[e] = 0.0;
    __syncthreads();
    const int trips = walk_lists<kListStride>(s_r1, s_list, count, p, tops, base);
    for (int i = 0; i < trips; ++i) {
      const int off = my_list[i];
      bool on;
      const float w = trip_weight(s_r0, s_r1, off, base, p, T, on);
      const float tot = row_transpose_sum<K>(w, mk, ms, p.j);  // lane j < K: channel j's sum of w map over the row's 16 pixels
      // every lane that holds a total adds it, zero or not (the sentinel slot's accumulators are never read)
      if (p.j < K)
        __hip_atomic_fetch_add((__attribute__((address_space(3))) double *)(&s_acc[(off >> 4) * K + p.j]), (double)tot,
                               __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    }
    __syncthreads();
    for (int e = tid; e < count * K; e += 256) {  // (slot, channel) = (e / K, e % K)
      const float tot = (float)s_acc[e];
      const int c = c0 + (e & (K - 1));
      if (tot != 0.0f && c < channels) atomicAdd(lifted + (size_t)a.c2g[s_gid[e / K]] * (size_t)channels + c, tot);
    }
  }
}

// ---- features backward: the feature map's gradient with respect to the GEOMETRY.  With G[p, c] = dL/d out[p, c] and
// d_i(p) = sum_c G[p, c] f[g_i, c], the map out[p, c] = sum_i w_ip f[g_i, c] is the forward's image with colours f, pixel
// gradient G and background 0, so d/d alpha_i(p) = T_i (d_i - s_i), s_i = the "colour behind" entry i dotted with G --
// render_bwd_kernel's ga with a C-vector per pixel.  The expression is linear in (f, G) over channels: every chunk of K
// channels walks the list with its own s and adds its own part.  The walk is render_bwd_kernel's, back to front from T_px
// (T rebuilt by the same rcp of 1 - the forward's capped alpha, gp = og ga with the uncapped og: the 0.99 cap is
// differentiated as if absent), on the full sorted / ranges / n_px, no compact lists and no segments, in batches of
// GS_BWD_BATCH (T comes from T_px, so the batches need not be the forward's).  Per trip a lane forms d_i as a K-term FMA
// chain over the staged feature row (K/4 broadcast reads), runs t = d_i - s, s = fma(alpha, t, s), and the six moments of
// gp about the tile centre are reduced over the row by row_moments6r (row_moments9r without the colour sums: lanes 0..2 of
// the totals are not added) and added with one ds_add_f64 per wave and trip into [slot][6] doubles.  Behind the batch one
// thread per gaussian forms row columns 3..8 exactly as render_bwd_kernel's flush does (same gate: nothing for
// sigmoid(opacity) == 1 or gp zero on the whole tile) and 16 lanes per gaussian add the non-zero ones to the gradient rows
// with float atomics (NaN goes out).  Columns 0..2 (the colours are the caller's: lift_features), 9 and the absgrad
// columns 10, 11 are never written.
// waves per SIMD the kernel is compiled for: five -- 84 / 88 / 96 VGPRs at K = 4 / 8 / 16, no scratch.  Occupancy is
// what it is bound by at K = 16: with row_moments9r on zero colour weights it held 98 VGPRs, four waves, and took
// 0.666 ms at C = 16 on config 3; held to five waves with two spilled registers 0.591 ms; asked for six every K spills
#ifndef GS_FEAT_BWD_WAVES
#define GS_FEAT_BWD_WAVES 5
#endif
template <int K>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(GS_FEAT_BWD_WAVES, 8))) void features_bwd_kernel(
    ReplayArgs a, int channels, const float *__restrict__ features, const float *__restrict__ grad_map, float *__restrict__ rows,
    int vec) {
  static_assert(K == 4 || K == 8 || K == 16, "chunk widths");
  constexpr int kB = GS_BWD_BATCH, kQ = K / 4, kAcc = 6;
  // r0 = (u, v, a2, b2), r1 = (c2, log2 opa, opa, block-hit bits); [kB]: the sentinel
  __shared__ float4 s_r0[kB + 1], s_r1[kB + 1];
  __shared__ float4 s_feat[(kB + 1) * kQ];    // [slot][K]; the sentinel's row is zeros
  __shared__ double s_acc[(kB + 1) * kAcc];   // [slot][S1, Sx, Sy, Sxx, Sxy, Syy]; doubles: see features_lift_kernel
  __shared__ int s_id[kB];
  // the row lists; dead once the batch's trips are done, and the flush parks its six values per gaussian on top of them
  __shared__ __attribute__((aligned(16))) unsigned short s_list[16 * kB + 2];
  static_assert(kB * kAcc * 4 <= 16 * kB * 2, "the flush values fit on the row lists");
  __shared__ int s_top;
  const int tile = ordered_tile(nullptr, (int)blockIdx.x, tile_count(a));
  if (tile >= tile_count(a)) return;
  const int c0 = (int)blockIdx.y * K;  // (more than one chunk: K = 16)
  const int tid = threadIdx.x;
  walk_setup<kB>(s_r0, s_r1, &s_top);
  if (tid < kQ) s_feat[kB * kQ + tid] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
  const TilePixel p = tile_pixel(a, tile);
  float T = p.inside ? a.T_px[p.pid] : 0.0f;
  float G[K];  // the pixel's gradient-map values of this chunk (an outside pixel: zeros, and it walks nothing)
  load_chunk<K>(grad_map, p, c0, channels, vec, G);
  WalkTops tops = walk_tops(p.n);
  __syncthreads();
  if (p.lane == 0) atomicMax(&s_top, tops.wave);
  __syncthreads();
  tops.tile = s_top;
  if (tops.tile <= 0) return;
  const char *r0b = reinterpret_cast<const char *>(s_r0), *r1b = reinterpret_cast<const char *>(s_r1);
  const char *fb = reinterpret_cast<const char *>(s_feat);
  float *s_res = reinterpret_cast<float *>(s_list);
  // where this lane's share of the row totals goes: row_moments9r's sums 3..8 are accumulators 0..5
  const int red_idx = row_moments9r_index(p.lane) - 3;
  const bool red_lane = red_idx >= 0;
  const unsigned int acc_lane =
      (unsigned int)(size_t)(__attribute__((address_space(3))) char *)reinterpret_cast<char *>(s_acc) + (unsigned int)(max(red_idx, 0) * 8);
  const float alpha_cap = __builtin_amdgcn_exp2f(kLog2AlphaMax);
  // the lane constants of the six moments: pixel position relative to the tile centre; no colour sums (weights 0)
  const RowsWeights rw = make_rows_weights(p.lane, p.fpx - (p.tx0 + 7.5f), p.fpy - (p.ty0 + 7.5f), 0.0f, 0.0f, 0.0f);
  const unsigned short *my_list = s_list + (p.wave * 4 + p.row) * kB;  // this row's of the wave's four lists
  float s = 0.0f;  // G . (features behind the current entry): background 0
  for (int base = ((tops.tile - 1) / kB) * kB; base >= 0; base -= kB) {
    const int count = min(kB, tops.tile - base);
    __syncthreads();  // the flush of the batch before has read the parked values and the ids
    if (tid < count) {
      SplatRec r;
      unsigned int hits;
      s_id[tid] = staged_entry(a, p, base + tid, r, hits);
      s_r0[tid] = r.r0;
      s_r1[tid] = make_float4(r.r1.x, r.r1.y, r.r1.z, __uint_as_float(hits));
    }
    gather_features<K>(a, p.start + base, count, c0, channels, features, reinterpret_cast<float *>(s_feat));
    for (int e = tid; e < count * kAcc; e += 256) s_acc[e] = 0.0;
    __syncthreads();
    if (base < tops.wave) {
      const int trips = walk_lists<kB>(s_r1, s_list, count, p, tops, base);
      for (int i = trips - 1; i >= 0; --i) {
        const int off = my_list[i];  // a row past the end of its list reads the sentinel record: alpha 0, features 0
        const float4 a0 = *reinterpret_cast<const float4 *>(r0b + off), b = *reinterpret_cast<const float4 *>(r1b + off);
        // the forward's alpha bit for bit: staged_alpha is its exponent chain, the cap is taken below
        float og = staged_alpha(a0.z, a0.w, b.x, b.y, a0.x - p.fpx, a0.y - p.fpy);
        // (n is 0 for pixels outside the image; "not below" lets a NaN pass, as in render_bwd_kernel)
        const bool valid = !(og < kAlphaMin) && base + (off >> 4) < p.n;
        if (__ballot(valid) == 0ull) continue;
        og = valid ? og : 0.0f;
        float alpha;  // v_exp_f32(kLog2AlphaMax): the cap the forward composed with (see render_bwd_kernel)
        asm("v_min_f32 %0, %2, %1" : "=v"(alpha) : "v"(og), "v"(alpha_cap));
        T *= __builtin_amdgcn_rcpf(1.0f - alpha);  // transmittance in front of this entry
        const float4 *f = reinterpret_cast<const float4 *>(fb + off * kQ);
        float d = 0.0f;  // d_i = sum_c G[c] f[c], one chain in channel order
#pragma unroll
        for (int q = 0; q < kQ; ++q) {
          const float4 v = f[q];
          d = q == 0 ? v.x * G[0] : __builtin_fmaf(v.x, G[4 * q], d);
          d = __builtin_fmaf(v.y, G[4 * q + 1], d);
          d = __builtin_fmaf(v.z, G[4 * q + 2], d);
          d = __builtin_fmaf(v.w, G[4 * q + 3], d);
        }
        const float t = d - s;
        const float ga = t * T;  // d/d alpha
        s = __builtin_fmaf(alpha, t, s);
        const float gp = og * ga;  // d/d power
        unsigned int acc_addr;
        const float red = row_moments6r<3>(gp, rw, (unsigned int)off, acc_lane, acc_addr);
        // every lane that holds a moment adds it, zero or not (rows past their list add zeros to the sentinel's slot)
        if (red_lane)
          __hip_atomic_fetch_add(reinterpret_cast<__attribute__((address_space(3))) double *>(acc_addr), (double)red,
                                 __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
      }
    }
    __syncthreads();
    // flush, step 1: one thread per gaussian turns its six moments into row columns 3..8 (render_bwd_kernel's flush)
    if (tid < count) {
      const double *acc = &s_acc[tid * kAcc];
      const float4 a0 = s_r0[tid], b = s_r1[tid];
      const float opa = b.z;
      const double X = (double)(a0.x - (p.tx0 + 7.5f)), Y = (double)(a0.y - (p.ty0 + 7.5f));
      const double S1 = acc[0], Sx = acc[1], Sy = acc[2];
      const float sx = (float)(X * S1 - Sx), sy = (float)(Y * S1 - Sy);
      const float sxx = (float)(X * (X * S1 - 2.0 * Sx) + acc[3]);
      const float sxy = (float)(X * (Y * S1 - Sy) - Y * Sx + acc[4]);
      const float syy = (float)(Y * (Y * S1 - 2.0 * Sy) + acc[5]);
      const float ca = a0.z * kConicDiag, cb = a0.w * kConicOff, cc = b.x * kConicDiag;
      const bool any_gp = (S1 != 0.0) | (Sx != 0.0) | (Sy != 0.0) | (acc[3] != 0.0) | (acc[4] != 0.0) | (acc[5] != 0.0);
      const float keep = (opa == 1.0f || !any_gp) ? 0.0f : 1.0f;
      float *res = &s_res[tid * kAcc];
      res[0] = keep * ((float)S1 * (1.0f - opa));
      res[1] = keep * (-0.5f * sxx);
      res[2] = keep * -sxy;
      res[3] = keep * (-0.5f * syy);
      res[4] = keep * (-(ca * sx + cb * sy) * (0.5f * (float)a.width));
      res[5] = keep * (-(cc * sy + cb * sx) * (0.5f * (float)a.height));
    }
    __syncthreads();
    // step 2: 16 lanes per gaussian, six of them with a column each
    if (p.j < kAcc) {
      for (int slot = tid >> 4; slot < count; slot += 16) {
        const float val = s_res[slot * kAcc + p.j];
        if (!(val != 0.0f)) continue;  // zero (nothing to add) -- NaN still goes out
        atomicAdd(&rows[(size_t)s_id[slot] * 16 + 3 + p.j], val);
      }
    }
  }
}

// ---- launchers (gs_launch.h) ----------------------------------------------------------------------------------------
int launch_contributions(const ReplayArgs &a, float *weight_sum, float *weight_max, int *pixels, hipStream_t st) {
  contributions_kernel<<<dim3(tile_grid(tile_count(a))), dim3(256), 0, st>>>(a, weight_sum,
                                                                             reinterpret_cast<unsigned int *>(weight_max), pixels);
  GS_LAUNCH_CHECK();
  return GSPLAT_OK;
}

int launch_median_depth(const ReplayArgs &a, const float *xyz_c, float threshold, float *depth, int *index, hipStream_t st) {
  median_depth_kernel<<<dim3(tile_grid(tile_count(a))), dim3(256), 0, st>>>(a, xyz_c, threshold, depth, index);
  GS_LAUNCH_CHECK();
  return GSPLAT_OK;
}

// A feature launch: f(K, grid, vec) with the chunk width K = the smallest of 4 / 8 / 16 that holds all channels, 16 beyond
// (gridDim.y chunks then), and vec = 16-byte accesses to the caller's [H,W,C] array `px_array`: C is a multiple of 4 and
// the array starts on 16 bytes.
template <class F>
static void with_chunks(const ReplayArgs &a, int channels, const void *px_array, F &&f) {
  const int vec = (channels & 3) == 0 && ((size_t)px_array & 15) == 0 ? 1 : 0;
  auto launch = [&](auto k) {
    constexpr int K = decltype(k)::value;
    f(k, dim3(tile_grid(tile_count(a)), (channels + K - 1) / K), vec);
  };
  if (channels <= 4) launch(std::integral_constant<int, 4>{});
  else if (channels <= 8) launch(std::integral_constant<int, 8>{});
  else launch(std::integral_constant<int, 16>{});
}

int launch_features_fwd(const ReplayArgs &a, int channels, const float *features, float *out, hipStream_t st) {
  with_chunks(a, channels, out, [&](auto k, dim3 grid, int vec) {
    features_fwd_kernel<decltype(k)::value><<<grid, dim3(256), 0, st>>>(a, channels, features, out, vec);
  });
  GS_LAUNCH_CHECK();
  return GSPLAT_OK;
}

int launch_features_lift(const ReplayArgs &a, int channels, const float *map, float *lifted, hipStream_t st) {
  with_chunks(a, channels, map, [&](auto k, dim3 grid, int vec) {
    features_lift_kernel<decltype(k)::value><<<grid, dim3(256), 0, st>>>(a, channels, map, lifted, vec);
  });
  GS_LAUNCH_CHECK();
  return GSPLAT_OK;
}

int launch_features_bwd(const ReplayArgs &a, int channels, const float *features, const float *grad_map, float *rows,
                        hipStream_t st) {
  with_chunks(a, channels, grad_map, [&](auto k, dim3 grid, int vec) {
    features_bwd_kernel<decltype(k)::value><<<grid, dim3(256), 0, st>>>(a, channels, features, grad_map, rows, vec);
  });
  GS_LAUNCH_CHECK();
  return GSPLAT_OK;
}

}  // namespace gs
