// gs_preprocess.hip -- the per-gaussian forward of the device-resident pass (gsplat_rasterize_image, gs_fused.hip):
// project_cull -> preprocess<L> (or its two-kernel forms, sh_colour + preprocess_geom) and, on the radix route, the record
// of the counts.  Kernels first, their launchers (gs_launch.h; arguments: gs_pergaussian_args.h) at the end.  Nothing here
// knows the context.
#include <cstring>
#include <rocprim/rocprim.hpp>

#include "gs_common.h"
#include "gs_launch.h"
#include "gs_math.h"
#include "gs_pergaussian_args.h"
#include "gs_render.h"
#include "gs_rows.h"

namespace {

constexpr int kBlock = 256;

// ---- A: world -> camera -> pixel -> keep-mask, for all N, and the compaction ranks
// kBinBlocks workgroups of kBinThreads; workgroup b owns the global indices of the chunks [C*b/kBinBlocks,
// C*(b+1)/kBinBlocks) (gs_common.h: bin_slice_first_chunk).  rank[i] leaves this kernel as the exclusive count of kept
// gaussians INSIDE the slice and slice_counts[b] as the slice's total; preprocess_kernel adds the counts of the slices
// before the gaussian's own and stores the global rank.  That replaces a two-kernel rocPRIM scan over N + 1 flags (12 us of
// launch + drain on the forward's critical path and 12 MB of traffic) by two barriers in a kernel that is here anyway.
// Pass 1 has no barrier, so the loads of all trips overlap; it leaves one ballot per (trip, wave) in LDS, wave 0 scans
// their counts, pass 2 only stores.
__global__ __launch_bounds__(gs::kBinThreads) void project_cull_kernel(const float *__restrict__ xyz,
                                                                       const float *__restrict__ view,
                                                                       const float *__restrict__ proj, int N, int width,
                                                                       int height, float near_thresh, int padding,
                                                                       float *__restrict__ xyz_c, float *__restrict__ uv,
                                                                       unsigned char *__restrict__ mask,
                                                                       int *__restrict__ rank,
                                                                       int *__restrict__ slice_counts,
                                                                       unsigned long long *__restrict__ pair_counters,
                                                                       int *__restrict__ kept,
                                                                       int *__restrict__ chunk_first) {
  extern __shared__ unsigned long long s_ballot[];  // [trips * 16] ballots, then [trips * 16] exclusive counts (int)
  constexpr int kWaves = gs::kBinThreads / 64;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int C = gs::bin_chunks(N);
  const int lo = gs::kBinChunk * gs::bin_slice_first_chunk(C, blockIdx.x);
  const int hi = min(N, gs::kBinChunk * gs::bin_slice_first_chunk(C, blockIdx.x + 1));
  const int trips = (hi - lo + gs::kBinThreads - 1) / gs::kBinThreads;
  int *s_before = reinterpret_cast<int *>(s_ballot + trips * kWaves);
  if (blockIdx.x == 0 && threadIdx.x < 64) pair_counters[threadIdx.x] = 0ull;  // consumed by preprocess_kernel
  const gs::Mat34 v = gs::load_view(view);
  const gs::Mat44 p = gs::load_proj(proj);
  for (int t = 0; t < trips; ++t) {
    const int i = lo + t * gs::kBinThreads + (int)threadIdx.x;
    bool k = false;
    if (i < hi) {
      float x, y, z, u, q;
      gs::camera_space(v, xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2], x, y, z);
      gs::to_screen(p, x, y, z, width, height, u, q);
      k = gs::keep(u, q, z, near_thresh, padding, width, height);
      if (xyz_c) {  // ForwardPassData's uncompacted d_xyz_c / d_uv; a lean context does not materialise them
        xyz_c[3 * i] = x; xyz_c[3 * i + 1] = y; xyz_c[3 * i + 2] = z;
        uv[2 * i] = u; uv[2 * i + 1] = q;
      }
      mask[i] = k ? 1 : 0;
    }
    const unsigned long long bal = __ballot(k);
    if (lane == 0) s_ballot[t * kWaves + w] = bal;
  }
  __syncthreads();
  if (w == 0) {  // exclusive scan of the trips * 16 ballot counts, slice order = (trip, wave)
    const int n = trips * kWaves, per = (n + 63) / 64;
    int sum = 0;
    for (int e = lane * per; e < min(lane * per + per, n); ++e) sum += __popcll(s_ballot[e]);
    int incl = sum;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
      const int u = __shfl_up(incl, off, 64);
      if (lane >= off) incl += u;
    }
    int run = incl - sum;
    for (int e = lane * per; e < min(lane * per + per, n); ++e) { s_before[e] = run; run += __popcll(s_ballot[e]); }
    if (lane == 63) slice_counts[blockIdx.x] = incl;
  }
  __syncthreads();
  for (int t = 0; t < trips; ++t) {
    const int i = lo + t * gs::kBinThreads + (int)threadIdx.x;
    if (i < hi) {
      const unsigned long long bal = s_ballot[t * kWaves + w];
      const int r = s_before[t * kWaves + w] + __popcll(bal & ((1ull << lane) - 1ull));
      rank[i] = r;
      // r06: the slice-local rank of every 64-entry chunk's first index (a slice starts on a chunk boundary and a trip is
      // sixteen chunks), for sh_colour_kernel when it runs BESIDE preprocess_geom_kernel, which rewrites rank[] in place
      if (chunk_first && lane == 0) chunk_first[(lo >> 6) + t * kWaves + w] = s_before[t * kWaves + w];
      // the slice's kept gaussians as a list (preprocess_kernel's compacted walk; null when the next kernel walks all)
      if (kept && ((bal >> lane) & 1ull)) kept[lo + r] = i;
    }
  }
}

// Rows of K floats of a wave's active lanes -- compacted positions p = 0 .. nact-1, consecutive global rows j0 + p -- staged in
// the wave's LDS area and written as ONE linear span of 16-byte stores, instead of K strided 4-byte stores per lane (r04).
// Measured on the forward that stores every ForwardPassData array (Sigma, J, conic, colour: 24 strided dword stores per
// gaussian more than the lean one): preprocess 0.132 -> 0.104 ms.  The lean kernel's own strided stores (the 48-byte record,
// the camera-space position) gain nothing from the same treatment (0.0885 -> 0.0883 .. 0.0909) and keep their direct form.
template <int K>
__device__ __forceinline__ void wave_rows_store(float *__restrict__ dst, int j0, int p, int nact, const float *v, float *wsh) {
#pragma unroll
  for (int k = 0; k < K; ++k) wsh[p * K + k] = v[k];
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  const int total = nact * K;
  float *out = dst + (size_t)j0 * K;
  for (int e = p * 4; e + 3 < total; e += nact * 4)
    *reinterpret_cast<gs::f4u *>(out + e) = __builtin_bit_cast(gs::f4u, *reinterpret_cast<const float4 *>(wsh + e));
  for (int e = (total & ~3) + p; e < total; e += nact) out[e] = wsh[e];
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");  // (the area is reused by the next array)
  __builtin_amdgcn_wave_barrier();
}

constexpr int kCoopTiles = 64;  // candidate tiles above which a splat's tile tests are shared by its wave

struct PreOut {
  int *c2g;
  float *xyz_c, *uv, *sigma, *conic, *J, *rgb, *radius;
  float4 *recs;
  int *counts;
  unsigned long long *hitmask;  // per gaussian: one bit per tile of its coarse rectangle (rectangles of <= 64 tiles)
  unsigned long long *pairs;  // 64 spread counters of coarse candidate pairs (reporting only)
  float *dir_sums;  // kDirSums: [M,9] gs::sh_dir_sums of every kept gaussian, for the per-gaussian backward
};

// ---- B: everything per kept gaussian, written at its compacted slot
// Launched as kBinBlocks workgroups of kBinThreads; workgroup b owns every kBinBlocks-th chunk of 64 entries
// (gs_common.h: kBinChunk).  When `table` is given it also histograms the tiles its gaussians hit in LDS -- the count
// phase of the counting-sort binning, for free next to the separating-axis tests -- and writes the row table[b][0..T).
//   kStoreMid: Sigma, J, conic and the SH colour are stored (ForwardPassData, cuda_data.cuh:70-86).  The fused backward
//     recomputes the first three and never reads the colour, so a training context that does not hand them to its
//     caller (gsplat_context_set_lean_forward) skips 72 of the 176 bytes this kernel writes per gaussian.
//   kCompact: the chunks are chunks of the M compacted slots, resolved through the slice-local lists project_cull_kernel
//     left in `kept` (kept[first index of slice s + k] = global index of the slice's k-th kept gaussian), instead of
//     chunks of all indices with the culled lanes idle: a view that culls every other gaussian runs half the trips
//     (r02: 23 % of HBM on such a view).
// Everything a gaussian stores leaves BEFORE its tile loop, which then holds six numbers per lane: kept across the loop,
// Sigma, J, conic, colour and the 48-byte record pushed the SH-3 instance past its 128 registers (6 spilled in r02).
//   kAntialias (gsplat_context_set_antialiased): the record's opacity is sigmoid(logit) * rho; conic, radii and tile tests
//     are what they are without the flag -- a template flag, so that the default instantiations stay exactly what they were
//   kDirSums (gsplat_context_set_dir_sums): the lane also forms gs::sh_dir_sums -- the nine sums over its coefficient row
//     that the position gradient through the view direction is made of -- while the row is in its registers for the colour,
//     and stores them at its compacted slot (36 bytes); preprocess_bwd_kernel<.., kDirSums> then reads those instead of the
//     row, band 0 and the camera-space position (204 bytes).  The sums are gs::sh_bwd's own, the same inlined code on the same
//     inputs.  Again a template flag: every other instantiation is what it was.
template <int L, bool kStoreMid, bool kCompact, bool kAntialias = false, bool kDirSums = false>
__global__ __launch_bounds__(gs::kBinThreads) void preprocess_kernel(gsplat_gaussians g, const float *__restrict__ view,
                                                            const unsigned char *__restrict__ mask,
                                                            int *__restrict__ rank,
                                                            const int *__restrict__ slice_counts,
                                                            const int *__restrict__ kept,
                                                            const float *__restrict__ proj, int width, int height,
                                                            float fx, float fy,
                                                            float tan_fovx, float tan_fovy, float mh_dist, float cx,
                                                            float cy, float cz, int ntx, int nty, PreOut o,
                                                            int *__restrict__ table) {
  extern __shared__ int s_hist[];
  __shared__ int s_base[gs::kBinBlocks + 1];  // kept gaussians before each of the cull's slices; [kBinBlocks]: all of them
  __shared__ int s_wsum[4];
  const int N = g.num_gaussians, T = ntx * nty;
  static_assert(gs::kBinBlocks == 256, "the scan below is written for four waves of slice counts");
  {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    int cnt = 0, incl = 0;
    if (threadIdx.x < gs::kBinBlocks) {
      cnt = slice_counts[threadIdx.x];
      incl = cnt;
#pragma unroll
      for (int off = 1; off < 64; off <<= 1) {
        const int u = __shfl_up(incl, off, 64);
        if (lane >= off) incl += u;
      }
      if (lane == 63) s_wsum[w] = incl;
    }
    if (table)
      for (int t = threadIdx.x; t < T; t += gs::kBinThreads) s_hist[t] = 0;
    __syncthreads();
    if (threadIdx.x < gs::kBinBlocks) {
      int before = 0;
      for (int q = 0; q < w; ++q) before += s_wsum[q];
      s_base[threadIdx.x] = before + incl - cnt;
      if (threadIdx.x == gs::kBinBlocks - 1) s_base[gs::kBinBlocks] = before + incl;
    }
    __syncthreads();
  }
  const int M = s_base[gs::kBinBlocks];
  const int C = gs::bin_chunks(N);  // chunks of the index space: the cull's slices are runs of them
  unsigned long long coarse = 0;
  const int lane = threadIdx.x & 63;
  // what a walk over all indices in order did on the side: counts[M..N] must read 0 in the scan that may follow, and
  // rank[N] holds the total
  for (long long i = (long long)M + (long long)blockIdx.x * gs::kBinThreads + threadIdx.x; i <= N;
       i += (long long)gs::kBinBlocks * gs::kBinThreads)
    o.counts[i] = 0;
  if (blockIdx.x == 0 && threadIdx.x == 0) rank[N] = M;
  // This workgroup's chunks, one wave trip each (gs_common.h): chunk c of the walked space -- all N indices, or the M
  // compacted slots (kCompact) -- belongs to workgroup c % kBinBlocks and to its wave (c / kBinBlocks) % 16.  The trip
  // count is wave-uniform: the tiles of LARGE splats are tested by the whole wave together (below).
  const int walk_chunks = gs::bin_chunks(kCompact ? M : N);
  for (int c = (int)blockIdx.x + gs::kBinBlocks * (int)(threadIdx.x >> 6); c < walk_chunks;
       c += gs::kBinBlocks * (gs::kBinThreads / 64)) {
  const int e = c * gs::kBinChunk + lane;  // kCompact: the compacted slot; else the global index
  int i = e, j = e;
  bool act;
  if constexpr (kCompact) {
    act = e < M;
    // the slice of the cull that holds compacted slot e: the last s with s_base[s] <= e (binary search in LDS)
    int sl = 0;
#pragma unroll
    for (int step = gs::kBinBlocks / 2; step > 0; step >>= 1) sl += (s_base[sl + step] <= e) ? step : 0;
    i = act ? kept[gs::kBinChunk * gs::bin_slice_first_chunk(C, sl) + (e - s_base[sl])] : 0;
    if (act) rank[i] = j;
  } else {
    // local -> global rank, for every index (the pack kernels read it through the mask, bin_scatter_kernel at the
    // chunk starts): a chunk lies inside one slice of the cull
    const int sl = gs::bin_slice_of_chunk(C, c);
    if (i < N) {
      j = s_base[sl] + rank[i];
      rank[i] = j;
    }
    act = i < N && mask[i];
  }
  int hits = 0, span_n = 0;
  unsigned long long hm = 0ull;
  float bu = 0.0f, bv = 0.0f, br0 = 0.0f, br1 = 0.0f, br2 = 0.0f, br3 = 0.0f;  // what the tile tests need of a lane
  if (act) {
    constexpr int n = (L + 1) * (L + 1);
    const gs::Mat34 vw = gs::load_view(view);
    // colour
    float dx, dy, dz, len, rgb[3];
    gs::view_dir(g.xyz[3 * i], g.xyz[3 * i + 1], g.xyz[3 * i + 2], cx, cy, cz, dx, dy, dz, len);
    if constexpr (kDirSums) {
      // The row and band 0 are loaded ONCE, into registers, and walked once for the colour and the sums.  Left to itself
      // the compiler forms the whole basis and all of its gradient while the 45 coefficients are in flight, next to twelve
      // accumulators, and the degree-3 kernels spill (10 to 69 registers, every form tried); scheduling barriers do not
      // hold arithmetic in place.  So the walk is tied together by data: at five points the direction and the running
      // sums pass through one empty asm, and nothing behind it can be formed before everything in front of it is summed.
      // Degree 3: 114 to 120 registers, no scratch (the kernel without the flag: 127 / 128).
      constexpr int kRow = (n - 1) * 3;
      float row[kRow > 0 ? kRow : 1], b0[3];
      {
        const float *src = g.sh + (size_t)i * kRow;
#pragma unroll
        for (int k = 0; k < kRow; ++k) row[k] = src[k];
        b0[0] = g.rgb[3 * i]; b0[1] = g.rgb[3 * i + 1]; b0[2] = g.rgb[3 * i + 2];
      }
      float ds[9];
      gs::sh_to_rgb_dir_sums<L>(row, b0, dx, dy, dz, rgb, ds, [](float &x, float &y, float &z, float *s, float &r, float &g, float &b) {
        asm volatile("" : "+v"(x), "+v"(y), "+v"(z), "+v"(s[0]), "+v"(s[1]), "+v"(s[2]), "+v"(s[3]), "+v"(s[4]), "+v"(s[5]),
                          "+v"(s[6]), "+v"(s[7]), "+v"(s[8]), "+v"(r), "+v"(g), "+v"(b));
      });
      float *dst = o.dir_sums + 9 * (size_t)j;  // (stored at once: nine registers that nothing below needs)
#pragma unroll
      for (int k = 0; k < 9; ++k) dst[k] = ds[k];
    } else {
      gs::sh_to_rgb<L>(g.sh + (size_t)i * (n - 1) * 3, g.rgb + 3 * i, dx, dy, dz, rgb);
    }
    // covariance -> conic
    const float4 q = reinterpret_cast<const float4 *>(g.quaternion)[i];
    const gs::RotScale rs = gs::rot_scale(q.x, q.y, q.z, q.w, g.scale[3 * i], g.scale[3 * i + 1], g.scale[3 * i + 2]);
    float sg[6], J[6], con[3], rad[4];
    gs::sigma_from(rs, sg);
    // kStoreMid: the stores go through the wave's staging area (wave_rows_store).  All active lanes of the wave are here
    // together: their compacted positions, and the row of the first one (the rows of a chunk's active lanes are consecutive)
    __shared__ __attribute__((aligned(16))) float s_stage[kStoreMid ? gs::kBinThreads / 64 : 1][kStoreMid ? 64 * 12 : 4];
    int pp = 0, nact = 0, j0 = 0;
    float *wsh = s_stage[0];
    if constexpr (kStoreMid) {
      const unsigned long long actm = __ballot(true);
      nact = __popcll(actm);
      pp = __popcll(actm & ((1ull << lane) - 1ull));
      j0 = __builtin_amdgcn_readfirstlane(j - pp);
      wsh = s_stage[threadIdx.x >> 6];
      // each of the four as soon as it exists: all of them pending at once cost spilled registers
      wave_rows_store<6>(o.sigma, j0, pp, nact, sg, wsh);
      wave_rows_store<3>(o.rgb, j0, pp, nact, rgb, wsh);
    }
    // camera-space position and pixel coordinates: recomputed with project_cull_kernel's functions on the same inputs
    // (bit for bit its values) from a second, cache-resident read of the position, instead of a 20-byte round trip
    // through the uncompacted arrays
    float x, y, z, u, v;
    {
      int i2 = i;
      asm volatile("" : "+v"(i2));  // an opaque copy: the first read's registers are not kept alive across the SH sum
      gs::camera_space(vw, g.xyz[3 * i2], g.xyz[3 * i2 + 1], g.xyz[3 * i2 + 2], x, y, z);
      gs::to_screen(gs::load_proj(proj), x, y, z, width, height, u, v);
    }
    gs::jacobian(x, y, z, fx, fy, tan_fovx, tan_fovy, J);
    [[maybe_unused]] float rho = 1.0f, cov_raw[3];
    if constexpr (kAntialias) gs::conic_radius<true>(J, sg, vw, mh_dist, con, rad, &rho, cov_raw);
    else gs::conic_radius(J, sg, vw, mh_dist, con, rad);
    // stores (compacted order); counts and hitmask follow the tile tests
    o.c2g[j] = i;
    o.uv[2 * j] = u; o.uv[2 * j + 1] = v;
    reinterpret_cast<float4 *>(o.radius)[j] = make_float4(rad[0], rad[1], rad[2], rad[3]);
    gs::SplatRec rec;
    if constexpr (kAntialias)
      rec = gs::make_record_opa(u, v, con[0], con[1], con[2], gs::sigmoid_fast(g.opacity[i]) * rho, rgb[0], rgb[1], rgb[2]);
    else
      rec = gs::make_record(u, v, con[0], con[1], con[2], g.opacity[i], rgb[0], rgb[1], rgb[2]);
    if constexpr (kStoreMid) {
      const float xyzc[3] = {x, y, z};
      wave_rows_store<3>(o.xyz_c, j0, pp, nact, xyzc, wsh);
      wave_rows_store<6>(o.J, j0, pp, nact, J, wsh);
      wave_rows_store<3>(o.conic, j0, pp, nact, con, wsh);
      const float rr[12] = {rec.r0.x, rec.r0.y, rec.r0.z, rec.r0.w, rec.r1.x, rec.r1.y, rec.r1.z, rec.r1.w,
                            rec.r2.x, rec.r2.y, rec.r2.z, rec.r2.w};
      wave_rows_store<12>(reinterpret_cast<float *>(o.recs), j0, pp, nact, rr, wsh);
    } else {
      o.xyz_c[3 * j] = x; o.xyz_c[3 * j + 1] = y; o.xyz_c[3 * j + 2] = z;
      o.recs[3 * j] = rec.r0; o.recs[3 * j + 1] = rec.r1; o.recs[3 * j + 2] = rec.r2;
    }
    bu = u; bv = v; br0 = rad[0]; br1 = rad[1]; br2 = rad[2]; br3 = rad[3];
  }
  if (act) {
    // exact tile count
    const gs::TileRect r = gs::coarse_rect(bu, bv, br0, ntx, nty);
    if (r.x1 > r.x0 && r.y1 > r.y0) {
      coarse += (unsigned long long)(r.x1 - r.x0) * (unsigned long long)(r.y1 - r.y0);
      const gs::Obb ob = gs::make_obb(bu, bv, br0, br1, br2, br3);
      const gs::TileRect sp = gs::obb_span(ob, r);
      const int rh = r.y1 - r.y0;
      span_n = max(0, sp.x1 - sp.x0) * max(0, sp.y1 - sp.y0);
      if (span_n <= kCoopTiles) {
        for (int tx = sp.x0; tx < sp.x1; ++tx)
          for (int ty = sp.y0; ty < sp.y1; ++ty) {
            const bool h = gs::obb_hits_tile(ob, tx, ty);
            const int bit = (tx - r.x0) * rh + (ty - r.y0);  // position in the full coarse rectangle
            hits += h ? 1 : 0;
            hm |= (h && bit < 64) ? (1ull << bit) : 0ull;  // read by the binning kernels when the rectangle has <= 64 tiles
            if (h && table) atomicAdd(&s_hist[ty * ntx + tx], 1);
          }
      }
    }
  }
  // Large splats (more than kCoopTiles candidate tiles after the axis-aligned clipping: a capture early in training has
  // gaussians over hundreds or thousands of tiles): one lane walking them alone decided the kernel's duration.  The
  // wave takes them one at a time: the owner's six numbers are broadcast, every lane rebuilds the same OBB (the same
  // functions on the same inputs: bit-identical decisions) and tests every 64th tile of the span.  Such splats have
  // rectangles of more than 64 tiles, so they carry no hit mask.
  for (unsigned long long big = __ballot(span_n > kCoopTiles); big != 0ull; big &= big - 1ull) {
    const int owner = __builtin_ctzll(big);
    const float ou = __shfl(bu, owner, 64), ov = __shfl(bv, owner, 64);
    const float o0 = __shfl(br0, owner, 64), o1 = __shfl(br1, owner, 64), o2 = __shfl(br2, owner, 64), o3 = __shfl(br3, owner, 64);
    const gs::TileRect r = gs::coarse_rect(ou, ov, o0, ntx, nty);
    const gs::Obb ob = gs::make_obb(ou, ov, o0, o1, o2, o3);
    const gs::TileRect sp = gs::obb_span(ob, r);
    const int sh = sp.y1 - sp.y0, total = (sp.x1 - sp.x0) * sh;
    int found = 0;
    for (int p = lane; p < total + lane; p += 64) {  // uniform trip count: every lane reaches the ballot
      bool h = false;
      if (p < total) {
        const int tx = sp.x0 + p / sh, ty = sp.y0 + p % sh;
        h = gs::obb_hits_tile(ob, tx, ty);
        if (h && table) atomicAdd(&s_hist[ty * ntx + tx], 1);
      }
      found += __popcll(__ballot(h));
    }
    if (lane == owner) hits = found;
  }
  if (act) {
    o.counts[j] = hits;
    o.hitmask[j] = hm;
  }
  }
  // candidate-pair count (what call 1 of get_sorted_gaussian_list reports): one atomic per wave, spread over 64
  // counters so that no single address serialises the chip
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) coarse += __shfl_down(coarse, off, 64);
  if ((threadIdx.x & 63) == 0 && coarse) atomicAdd(&o.pairs[(blockIdx.x * 16 + (threadIdx.x >> 6)) & 63], coarse);
  if (table) {
    __syncthreads();
    for (int t = threadIdx.x; t < T; t += gs::kBinThreads) table[(size_t)blockIdx.x * T + t] = s_hist[t];
  }
}

// ---- r06: the per-gaussian forward as TWO kernels (gsplat_context_set_preprocess_split / GSPLAT_PRE_SPLIT) ------------
// VERDICT r05 asked for the split that r04 had only priced: preprocess_kernel<3> needs 99-128 VGPRs (four waves per SIMD in
// the 1024-thread shape of the LDS histogram) and reaches 36 % of HBM on its algorithmic bytes.  Built here, bit-identical
// (tests/test_fused_gpu.py: test_preprocess_split_is_bit_identical), switchable -- and NOT the default, because it loses
// (profiles/r06_ab_preprocess_split.txt, same box, alternating):
//   sh_colour_kernel        SH -> colour as a plain stream: every wave moves its 64 rows (180 B each at degree 3) through
//                           LDS as one linear span of 16-byte loads (gs_rows.h), writes 12 bytes per gaussian.
//                           47 us for 228 MB = 4.8 TB/s.
//   preprocess_geom_kernel  everything else in the persistent 256 x 1024 shape; a gaussian's inputs are 14 dwords, so the
//                           chunk loop requests the next chunk's inputs a whole trip early, in front of the tile loop,
//                           and defers the tile count / hit mask stores to the next trip (one wait per trip, on loads
//                           and stores that are a tile loop old).  64 us lean / 69 us full.
//   mode 1 (one behind the other) 112 / 121 us against the fused kernel's 86 / 103; mode 2 (side by side on two streams,
//   the colour written straight into the records) 124 / 140: the geometry kernel slows down beside a stream of loads.
// Where the geometry kernel's 64 us go (diagnostic builds, profiles/r06_ab_preprocess_split.txt): without its tile loop
// 42 us, without tile loop and conic / radius arithmetic 40 us -- the floor is 150 MB, two thirds of it WRITTEN, at
// 3.7 TB/s, and the order of loads and stores inside a trip does not move it (three orders measured).  The fused kernel
// moves 350 MB (lean) in 86 us = 4.1 TB/s and 420 MB (every array stored) in 103 us: it already runs at the rate this
// mix of strided 4..16-byte stores reaches, with the SH loads riding in the shadow of the arithmetic; the figure the
// verdict compares it with, preprocess_bwd's 72 %, is a kernel whose traffic is linear spans read and written in equal
// parts.  What is left in the fused kernel is its tile loop (9 us) and bytes (the tile count array, 4 B, is dead weight
// on the sparse route).  cuda/raster.cu:78-100 runs the colour and the covariance chain as separate kernels too.
// `rank`: the cull's slice-local ranks (sequential form, in front of preprocess_geom_kernel) or, when the kernel runs
// beside that one -- which rewrites rank[] in place --, null: the rank then comes from `chunk_first` and the chunk's mask
// ballot.  `recs`: the colour goes into the 48-byte records (r2.xyz; the geometry kernel writes the rest of the record,
// r2.w included: disjoint bytes), `rgb_out`: and / or into ForwardPassData's colour array.
template <int L, bool kCompact>
__global__ __launch_bounds__(kBlock) void sh_colour_kernel(gsplat_gaussians g, const unsigned char *__restrict__ mask,
                                                           const int *__restrict__ rank,
                                                           const int *__restrict__ chunk_first,
                                                           const int *__restrict__ slice_counts,
                                                           const int *__restrict__ kept, float cx, float cy, float cz,
                                                           float *__restrict__ rgb_out, float4 *__restrict__ recs) {
  constexpr int n = (L + 1) * (L + 1), kRest = (n - 1) * 3;
  static_assert(kRest > 0, "degree 0 has no rest coefficients: preprocess_geom_kernel forms the colour itself");
  static_assert(gs::kBinBlocks == kBlock, "one thread per slice of the cull in the scan below");
  __shared__ __attribute__((aligned(16))) float s_sh[kBlock * kRest];
  __shared__ int s_base[gs::kBinBlocks + 1];
  __shared__ int s_wsum[4];
  const int N = g.num_gaussians;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  {  // kept gaussians before each of the cull's slices (as preprocess_kernel)
    const int cnt = slice_counts[threadIdx.x];
    int incl = cnt;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
      const int u = __shfl_up(incl, off, 64);
      if (lane >= off) incl += u;
    }
    if (lane == 63) s_wsum[w] = incl;
    __syncthreads();
    int before = 0;
    for (int q = 0; q < w; ++q) before += s_wsum[q];
    s_base[threadIdx.x] = before + incl - cnt;
    if (threadIdx.x == gs::kBinBlocks - 1) s_base[gs::kBinBlocks] = before + incl;
    __syncthreads();
  }
  const int M = s_base[gs::kBinBlocks];
  const int C = gs::bin_chunks(N);
  const int c = (int)blockIdx.x * (kBlock / 64) + w;  // this wave's chunk of the walked space
  if (c >= gs::bin_chunks(kCompact ? M : N)) return;
  const int e = c * gs::kBinChunk + lane;
  int i = e, j = e;
  bool act;
  if constexpr (kCompact) {
    act = e < M;
    int sl = 0;
#pragma unroll
    for (int step = gs::kBinBlocks / 2; step > 0; step >>= 1) sl += (s_base[sl + step] <= e) ? step : 0;
    i = act ? kept[gs::kBinChunk * gs::bin_slice_first_chunk(C, sl) + (e - s_base[sl])] : 0;
  } else {
    act = i < N && mask[i];
  }
  const unsigned long long actm = __ballot(act);
  if (actm == 0ull) return;
  if constexpr (!kCompact) {
    if (rank) {
      if (i < N) j = s_base[gs::bin_slice_of_chunk(C, c)] + rank[i];  // rank[]: still the cull's slice-local counts
    } else {
      j = s_base[gs::bin_slice_of_chunk(C, c)] + chunk_first[c] + __popcll(actm & ((1ull << lane) - 1ull));
    }
  }
  float *wsh = s_sh + (threadIdx.x - lane) * kRest;
  // position and band 0 of the lane's own gaussian: requested before the rows, used behind them
  float px = 0.0f, py = 0.0f, pz = 0.0f, b0[3] = {0.0f, 0.0f, 0.0f};
  if (act) {
    px = g.xyz[3 * i]; py = g.xyz[3 * i + 1]; pz = g.xyz[3 * i + 2];
    b0[0] = g.rgb[3 * i]; b0[1] = g.rgb[3 * i + 1]; b0[2] = g.rgb[3 * i + 2];
  }
  if (!kCompact && __popcll(actm) * 2 >= min(64, N - c * gs::kBinChunk)) {
    // a chunk of consecutive indices of which most are kept: one linear span, culled rows included
    gs::rows_to_lds<kRest>(g.sh + (size_t)c * gs::kBinChunk * kRest, wsh, min(64, N - c * gs::kBinChunk), lane);
  } else {
    // scattered rows (the compacted walk, or a chunk most of which is culled): twelve lanes fetch one row in 16-byte
    // pieces, all of a wave's loads issued before the first LDS store (as preprocess_bwd_kernel)
    constexpr int kPieces = (kRest + 3) / 4, kPer = 64 / kPieces, kIter = (64 + kPer - 1) / kPer;
    const int grp = lane / kPieces, piece = lane - grp * kPieces;
    const bool in_grp = grp < kPer;
    float4 v[kIter];
#pragma unroll
    for (int it = 0; it < kIter; ++it) {
      const int r = it * kPer + grp;
      const int ir = __shfl(i, r < 64 ? r : 0, 64);
      const bool want = in_grp && r < 64 && ((actm >> r) & 1ull);
      v[it] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
      if (want) {
        const float *src = g.sh + (size_t)ir * kRest + 4 * piece;
        if (4 * piece + 3 < kRest) {
          v[it] = __builtin_bit_cast(float4, *reinterpret_cast<const gs::f4u *>(src));
        } else {
          v[it].x = src[0];
          if (4 * piece + 1 < kRest) v[it].y = src[1];
          if (4 * piece + 2 < kRest) v[it].z = src[2];
        }
      }
    }
#pragma unroll
    for (int it = 0; it < kIter; ++it) {
      const int r = it * kPer + grp;
      if (in_grp && r < 64 && ((actm >> r) & 1ull)) {
        float *dst = wsh + r * kRest + 4 * piece;
        dst[0] = v[it].x;
        if (4 * piece + 1 < kRest) dst[1] = v[it].y;
        if (4 * piece + 2 < kRest) dst[2] = v[it].z;
        if (4 * piece + 3 < kRest) dst[3] = v[it].w;
      }
    }
  }
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_wave_barrier();
  if (act) {
    float dx, dy, dz, len, rgb[3];
    gs::view_dir(px, py, pz, cx, cy, cz, dx, dy, dz, len);
    gs::sh_to_rgb<L>(wsh + lane * kRest, b0, dx, dy, dz, rgb);
    if (rgb_out) { rgb_out[3 * j] = rgb[0]; rgb_out[3 * j + 1] = rgb[1]; rgb_out[3 * j + 2] = rgb[2]; }
    if (recs) {
      float *r2 = reinterpret_cast<float *>(recs + 3 * (size_t)j + 2);
      r2[0] = rgb[0]; r2[1] = rgb[1]; r2[2] = rgb[2];
    }
  }
}

// what a lane of preprocess_geom_kernel holds for a chunk it has not started yet
struct GeomData { float x, y, z, sx, sy, sz, op; float4 q; };

// kColour 0: degree 0 -- the colour is band 0 alone, formed here (no sh_colour_kernel); 1: read from o.rgb, where
// sh_colour_kernel has left it (the two kernels one behind the other); 2: none -- sh_colour_kernel runs BESIDE this kernel
// on a stream of its own and writes the colour into the records itself; this kernel stores r0, r1 and r2.w only
template <int kColour, bool kStoreMid, bool kCompact>
__global__ __launch_bounds__(gs::kBinThreads) void preprocess_geom_kernel(gsplat_gaussians g, const float *__restrict__ view,
                                                                  const unsigned char *__restrict__ mask,
                                                                  int *__restrict__ rank,
                                                                  const int *__restrict__ slice_counts,
                                                                  const int *__restrict__ kept,
                                                                  const float *__restrict__ proj, int width, int height,
                                                                  float fx, float fy, float tan_fovx, float tan_fovy,
                                                                  float mh_dist, float cx, float cy, float cz, int ntx,
                                                                  int nty, PreOut o, int *__restrict__ table) {
  extern __shared__ int s_hist[];
  __shared__ int s_base[gs::kBinBlocks + 1];
  __shared__ int s_wsum[4];
  __shared__ __attribute__((aligned(16))) float s_stage[kStoreMid ? gs::kBinThreads / 64 : 1][kStoreMid ? 64 * 12 : 4];
  const int N = g.num_gaussians, T = ntx * nty;
  static_assert(gs::kBinBlocks == 256, "the scan below is written for four waves of slice counts");
  {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    int cnt = 0, incl = 0;
    if (threadIdx.x < gs::kBinBlocks) {
      cnt = slice_counts[threadIdx.x];
      incl = cnt;
#pragma unroll
      for (int off = 1; off < 64; off <<= 1) {
        const int u = __shfl_up(incl, off, 64);
        if (lane >= off) incl += u;
      }
      if (lane == 63) s_wsum[w] = incl;
    }
    if (table)
      for (int t = threadIdx.x; t < T; t += gs::kBinThreads) s_hist[t] = 0;
    __syncthreads();
    if (threadIdx.x < gs::kBinBlocks) {
      int before = 0;
      for (int q = 0; q < w; ++q) before += s_wsum[q];
      s_base[threadIdx.x] = before + incl - cnt;
      if (threadIdx.x == gs::kBinBlocks - 1) s_base[gs::kBinBlocks] = before + incl;
    }
    __syncthreads();
  }
  const int M = s_base[gs::kBinBlocks];
  const int C = gs::bin_chunks(N);
  unsigned long long coarse = 0;
  const int lane = threadIdx.x & 63;
  for (long long i = (long long)M + (long long)blockIdx.x * gs::kBinThreads + threadIdx.x; i <= N;
       i += (long long)gs::kBinBlocks * gs::kBinThreads)
    o.counts[i] = 0;
  if (blockIdx.x == 0 && threadIdx.x == 0) rank[N] = M;
  const int walk_chunks = gs::bin_chunks(kCompact ? M : N);
  constexpr int kStep = gs::kBinBlocks * (gs::kBinThreads / 64);
  const int c_first = (int)blockIdx.x + gs::kBinBlocks * (int)(threadIdx.x >> 6);
  // The pipeline.  s_waitcnt vmcnt counts a wave's loads AND stores in issue order on gfx950: waiting for a load that was
  // issued behind stores waits for those stores' acknowledgements too, and a value's first use is where the compiler puts
  // the wait.  So everything a chunk needs from memory is REQUESTED one trip early, at the top of the trip, in front of
  // that trip's thirteen stores, and left untouched until the chunk's own trip begins: by then the loads are a whole
  // trip old and the wait lets the younger stores stay in flight (r05's kernel waited three times per trip with all of
  // its earlier stores still queued in front of the loads).
  auto load_data = [&](int i) {
    GeomData d;
    d.x = g.xyz[3 * i]; d.y = g.xyz[3 * i + 1]; d.z = g.xyz[3 * i + 2];
    d.q = reinterpret_cast<const float4 *>(g.quaternion)[i];
    d.sx = g.scale[3 * i]; d.sy = g.scale[3 * i + 1]; d.sz = g.scale[3 * i + 2];
    d.op = g.opacity[i];
    return d;
  };
  const GeomData kNoData = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, make_float4(0.0f, 0.0f, 0.0f, 0.0f)};
  // all indices in order: a chunk's data are at its own indices (requested whether kept or not: this walk runs when at
  // most a fifth is culled), rank[] and mask[] are requested with them.  compacted walk: the chunk's global indices come
  // from `kept`, requested TWO trips early (the data loads of the trip in between take them as addresses).
  int rk_n = 0, mk_n = 0, ix_n = 0, ix_nn = 0;  // raw: rank / mask of the next chunk | kept index of the next, next-next
  GeomData d_n = kNoData;
  auto kept_index = [&](int c) {  // global index of this lane's slot in chunk c of the compacted slots (0 past the end)
    const int e = c * gs::kBinChunk + lane;
    if (c >= walk_chunks || e >= M) return 0;
    int sl = 0;
#pragma unroll
    for (int step = gs::kBinBlocks / 2; step > 0; step >>= 1) sl += (s_base[sl + step] <= e) ? step : 0;
    return kept[gs::kBinChunk * gs::bin_slice_first_chunk(C, sl) + (e - s_base[sl])];
  };
  auto request = [&](int c) {  // the loads of chunk c (the chunk after the one being worked on)
    rk_n = 0; mk_n = 0; d_n = kNoData;
    const int e = c * gs::kBinChunk + lane;
    if constexpr (kCompact) {
      if (c < walk_chunks && e < M) d_n = load_data(ix_n);
    } else {
      if (c < walk_chunks && e < N) { rk_n = rank[e]; mk_n = mask[e]; d_n = load_data(e); }
    }
  };
  if constexpr (kCompact) { ix_n = kept_index(c_first); }
  request(c_first);
  if constexpr (kCompact) { ix_nn = kept_index(c_first + kStep); }
  bool late_act = false;  // the previous chunk's tile count and hit mask, stored with this trip's stores
  int late_j = 0, late_hits = 0;
  unsigned long long late_hm = 0ull;
  for (int c = c_first; c < walk_chunks; c += kStep) {
  // this chunk's values (requested a trip ago, in front of the previous tile loop)
  const int e0 = c * gs::kBinChunk + lane;
  const int rk = rk_n, mk = mk_n, i = kCompact ? ix_n : e0;
  const GeomData cur = d_n;
  bool act;
  int j = e0;
  if constexpr (kCompact) {
    act = e0 < M;
  } else {
    act = e0 < N && mk != 0;
    if (e0 < N) j = s_base[gs::bin_slice_of_chunk(C, c)] + rk;  // local -> global rank, for every index (see preprocess_kernel)
  }
  int hits = 0, span_n = 0;
  unsigned long long hm = 0ull;
  float bu = 0.0f, bv = 0.0f, br0 = 0.0f, br1 = 0.0f, br2 = 0.0f, br3 = 0.0f;
  if (act) {
    const gs::Mat34 vw = gs::load_view(view);
    // the colour: requested here, used when the record is made
    float rgb[3] = {0.0f, 0.0f, 0.0f};
    if constexpr (kColour == 0) {
      float dx, dy, dz, len;
      gs::view_dir(cur.x, cur.y, cur.z, cx, cy, cz, dx, dy, dz, len);
      gs::sh_to_rgb<0>(nullptr, g.rgb + 3 * i, dx, dy, dz, rgb);
    } else if constexpr (kColour == 1) {
      rgb[0] = o.rgb[3 * j]; rgb[1] = o.rgb[3 * j + 1]; rgb[2] = o.rgb[3 * j + 2];
    }
    const gs::RotScale rs = gs::rot_scale(cur.q.x, cur.q.y, cur.q.z, cur.q.w, cur.sx, cur.sy, cur.sz);
    float sg[6], J[6], con[3], rad[4];
    gs::sigma_from(rs, sg);
    int pp = 0, nact = 0, j0 = 0;
    float *wsh = s_stage[0];
    if constexpr (kStoreMid) {
      const unsigned long long actm = __ballot(true);
      nact = __popcll(actm);
      pp = __popcll(actm & ((1ull << lane) - 1ull));
      j0 = __builtin_amdgcn_readfirstlane(j - pp);
      wsh = s_stage[threadIdx.x >> 6];
      wave_rows_store<6>(o.sigma, j0, pp, nact, sg, wsh);
    }
    float x, y, z, u, v;
    gs::camera_space(vw, cur.x, cur.y, cur.z, x, y, z);
    gs::to_screen(gs::load_proj(proj), x, y, z, width, height, u, v);
    gs::jacobian(x, y, z, fx, fy, tan_fovx, tan_fovy, J);
    gs::conic_radius(J, sg, vw, mh_dist, con, rad);
    o.c2g[j] = i;
    o.uv[2 * j] = u; o.uv[2 * j + 1] = v;
    reinterpret_cast<float4 *>(o.radius)[j] = make_float4(rad[0], rad[1], rad[2], rad[3]);
    const gs::SplatRec rec = gs::make_record(u, v, con[0], con[1], con[2], cur.op, rgb[0], rgb[1], rgb[2]);
    if constexpr (kStoreMid) {
      const float xyzc[3] = {x, y, z};
      wave_rows_store<3>(o.xyz_c, j0, pp, nact, xyzc, wsh);
      wave_rows_store<6>(o.J, j0, pp, nact, J, wsh);
      wave_rows_store<3>(o.conic, j0, pp, nact, con, wsh);
      if constexpr (kColour == 0) wave_rows_store<3>(o.rgb, j0, pp, nact, rgb, wsh);
      if constexpr (kColour == 2) {  // (the colour's twelve bytes of the record belong to sh_colour_kernel)
        o.recs[3 * j] = rec.r0; o.recs[3 * j + 1] = rec.r1;
        reinterpret_cast<float *>(o.recs + 3 * (size_t)j + 2)[3] = rec.r2.w;
      } else {
        const float rr[12] = {rec.r0.x, rec.r0.y, rec.r0.z, rec.r0.w, rec.r1.x, rec.r1.y, rec.r1.z, rec.r1.w,
                              rec.r2.x, rec.r2.y, rec.r2.z, rec.r2.w};
        wave_rows_store<12>(reinterpret_cast<float *>(o.recs), j0, pp, nact, rr, wsh);
      }
    } else {
      o.xyz_c[3 * j] = x; o.xyz_c[3 * j + 1] = y; o.xyz_c[3 * j + 2] = z;
      o.recs[3 * j] = rec.r0; o.recs[3 * j + 1] = rec.r1;
      if constexpr (kColour == 2) reinterpret_cast<float *>(o.recs + 3 * (size_t)j + 2)[3] = rec.r2.w;
      else o.recs[3 * j + 2] = rec.r2;
    }
    bu = u; bv = v; br0 = rad[0]; br1 = rad[1]; br2 = rad[2]; br3 = rad[3];
  }
  // the rest of the trip's stores -- the global rank (every index: the pack kernels read it through the mask) and the
  // PREVIOUS chunk's tile count and hit mask, which its tile loop produced behind that trip's stores --, then the next
  // chunk's requests, then the tile loop: no memory instruction in it, so when the loop top waits for the requests,
  // everything this wave has in flight is a tile loop old
  if constexpr (kCompact) {
    if (act) rank[i] = j;
  } else {
    if (e0 < N) rank[e0] = j;
  }
  if (late_act) {
    o.counts[late_j] = late_hits;
    o.hitmask[late_j] = late_hm;
  }
  asm volatile("" ::: "memory");
  if constexpr (kCompact) { ix_n = ix_nn; }
  request(c + kStep);
  if constexpr (kCompact) { ix_nn = kept_index(c + 2 * kStep); }
  asm volatile("" ::: "memory");
  if (act) {
    const gs::TileRect r = gs::coarse_rect(bu, bv, br0, ntx, nty);
    if (r.x1 > r.x0 && r.y1 > r.y0) {
      coarse += (unsigned long long)(r.x1 - r.x0) * (unsigned long long)(r.y1 - r.y0);
      const gs::Obb ob = gs::make_obb(bu, bv, br0, br1, br2, br3);
      const gs::TileRect sp = gs::obb_span(ob, r);
      const int rh = r.y1 - r.y0;
      span_n = max(0, sp.x1 - sp.x0) * max(0, sp.y1 - sp.y0);
      if (span_n <= kCoopTiles) {
        for (int tx = sp.x0; tx < sp.x1; ++tx)
          for (int ty = sp.y0; ty < sp.y1; ++ty) {
            const bool h = gs::obb_hits_tile(ob, tx, ty);
            const int bit = (tx - r.x0) * rh + (ty - r.y0);
            hits += h ? 1 : 0;
            hm |= (h && bit < 64) ? (1ull << bit) : 0ull;
            if (h && table) atomicAdd(&s_hist[ty * ntx + tx], 1);
          }
      }
    }
  }
  for (unsigned long long big = __ballot(span_n > kCoopTiles); big != 0ull; big &= big - 1ull) {  // (as preprocess_kernel)
    const int owner = __builtin_ctzll(big);
    const float ou = __shfl(bu, owner, 64), ov = __shfl(bv, owner, 64);
    const float o0 = __shfl(br0, owner, 64), o1 = __shfl(br1, owner, 64), o2 = __shfl(br2, owner, 64), o3 = __shfl(br3, owner, 64);
    const gs::TileRect r = gs::coarse_rect(ou, ov, o0, ntx, nty);
    const gs::Obb ob = gs::make_obb(ou, ov, o0, o1, o2, o3);
    const gs::TileRect sp = gs::obb_span(ob, r);
    const int sh = sp.y1 - sp.y0, total = (sp.x1 - sp.x0) * sh;
    int found = 0;
    for (int p = lane; p < total + lane; p += 64) {
      bool h = false;
      if (p < total) {
        const int tx = sp.x0 + p / sh, ty = sp.y0 + p % sh;
        h = gs::obb_hits_tile(ob, tx, ty);
        if (h && table) atomicAdd(&s_hist[ty * ntx + tx], 1);
      }
      found += __popcll(__ballot(h));
    }
    if (lane == owner) hits = found;
  }
  late_act = act; late_j = j; late_hits = hits; late_hm = hm;
  }
  if (late_act) {
    o.counts[late_j] = late_hits;
    o.hitmask[late_j] = late_hm;
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) coarse += __shfl_down(coarse, off, 64);
  if ((threadIdx.x & 63) == 0 && coarse) atomicAdd(&o.pairs[(blockIdx.x * 16 + (threadIdx.x >> 6)) & 63], coarse);
  if (table) {
    __syncthreads();
    for (int t = threadIdx.x; t < T; t += gs::kBinThreads) table[(size_t)blockIdx.x * T + t] = s_hist[t];
  }
}

// {M, S, candidate pairs} gathered into one 16-byte record so that the forward's only read-back is one copy
__global__ __launch_bounds__(64) void publish_counts_kernel(const int *__restrict__ rank_total,
                                                            const int *__restrict__ offsets_total,
                                                            const unsigned long long *__restrict__ pair_counters,
                                                            volatile unsigned long long *out,
                                                            unsigned long long ticket) {
  // `out` is pinned host memory mapped into the device: the host polls it for its ticket instead of paying a
  // copy + stream synchronisation, and the kernels queued behind this one keep the GPU busy meanwhile
  unsigned long long v = pair_counters[threadIdx.x];
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
  if (threadIdx.x == 0)
    gs::publish_record(out, ticket, (unsigned int)*rank_total, (unsigned int)*offsets_total, v, 0u);
}

}  // namespace

namespace gs {

int launch_project_cull(const CullArgs &a, hipStream_t st) {
  // LDS of the cull: one ballot + one count per (trip, wave) of the largest slice (a run of whole 64-entry chunks)
  const size_t slice_max = ((size_t)bin_chunks(a.N) / kBinBlocks + 2) * kBinChunk;
  const size_t trips = (slice_max + kBinThreads - 1) / kBinThreads + 1;
  project_cull_kernel<<<kBinBlocks, kBinThreads, trips * (kBinThreads / 64) * 12, st>>>(
      a.xyz, a.view, a.proj, a.N, a.width, a.height, a.near_thresh, a.padding, a.xyz_c, a.uv, a.mask, a.rank,
      a.slice_counts, a.pair_counters, a.kept, a.chunk_first);
  GS_LAUNCH_CHECK();
  return GSPLAT_OK;
}

// preprocess_kernel and preprocess_geom_kernel take the same arguments in the same shape: kBinBlocks workgroups of
// kBinThreads, the tile histogram (counting-sort route) as dynamic LDS
template <class Kernel>
static void launch_per_gaussian(Kernel kernel, const PreprocessArgs &a, hipStream_t st) {
  const PreOut o = {a.c2g, a.xyz_c, a.uv, a.sigma, a.conic, a.J, a.rgb, a.radius, a.recs, a.counts, a.hitmask, a.pairs,
                    a.dir_sums};
  const size_t hist_bytes = a.table ? (size_t)a.ntx * a.nty * sizeof(int) : 0;
  kernel<<<kBinBlocks, kBinThreads, hist_bytes, st>>>(a.g, a.view, a.mask, a.rank, a.slice_counts, a.kept, a.proj, a.width,
                                                      a.height, a.fx, a.fy, a.tan_fovx, a.tan_fovy, a.mh_dist, a.campos[0],
                                                      a.campos[1], a.campos[2], a.ntx, a.nty, o, a.table);
}

int launch_preprocess(const PreprocessArgs &a, hipStream_t st) {
  GS_REQUIRE(!(a.antialiased && a.dir_sums), "the anti-aliased forward has no form that writes the direction sums");
  with_degree<0>(a.l_max, [&](auto L) {
    with_bool(a.store_mid, [&](auto mid) {
      with_bool(a.compact, [&](auto cmp) {
        constexpr int kL = decltype(L)::value;
        constexpr bool kMid = decltype(mid)::value, kCmp = decltype(cmp)::value;
        if (a.antialiased) launch_per_gaussian(preprocess_kernel<kL, kMid, kCmp, true>, a, st);
        else if (a.dir_sums) launch_per_gaussian(preprocess_kernel<kL, kMid, kCmp, false, true>, a, st);
        else launch_per_gaussian(preprocess_kernel<kL, kMid, kCmp, false>, a, st);
      });
    });
  });
  GS_LAUNCH_CHECK();
  return GSPLAT_OK;
}

int launch_preprocess_geom(const PreprocessArgs &a, int colour, hipStream_t st) {
  GS_REQUIRE(colour >= 0 && colour <= 2, "colour: 0 formed here, 1 read from rgb, 2 written by sh_colour_kernel");
  auto with_colour = [&](auto f) {
    if (colour == 0) f(std::integral_constant<int, 0>{});
    else if (colour == 1) f(std::integral_constant<int, 1>{});
    else f(std::integral_constant<int, 2>{});
  };
  with_colour([&](auto col) {
    with_bool(a.store_mid, [&](auto mid) {
      with_bool(a.compact, [&](auto cmp) {
        launch_per_gaussian(preprocess_geom_kernel<decltype(col)::value, decltype(mid)::value, decltype(cmp)::value>, a, st);
      });
    });
  });
  GS_LAUNCH_CHECK();
  return GSPLAT_OK;
}

int launch_sh_colour(const ShColourArgs &a, hipStream_t st) {
  GS_REQUIRE(a.l_max >= 1, "degree 0 has no colour kernel: preprocess_geom_kernel forms the colour itself");
  const dim3 grid(div_up(bin_chunks(a.g.num_gaussians), kBlock / 64)), block(kBlock);
  with_degree<1>(a.l_max, [&](auto L) {
    with_bool(a.compact, [&](auto cmp) {
      sh_colour_kernel<decltype(L)::value, decltype(cmp)::value><<<grid, block, 0, st>>>(
          a.g, a.mask, a.rank, a.chunk_first, a.slice_counts, a.kept, a.campos[0], a.campos[1], a.campos[2], a.rgb_out, a.recs);
    });
  });
  GS_LAUNCH_CHECK();
  return GSPLAT_OK;
}

// Temporary storage of rocPRIM's exclusive scan over the N + 1 tile counts (gs::scan_counts runs it between
// preprocess_kernel and publish_counts_kernel on the radix route; gsplat_context_create sizes the workspace with this).
// The query also instantiates the scan's kernels in THIS translation unit, where nothing launches them -- and that is why
// it lives here and not beside the context: with them in the module the compiler forms the lane index of __shfl_down in
// preprocess_kernel, preprocess_geom_kernel and publish_counts_kernel as (lane << 2) | 0x80 ...; without them it takes an
// equivalent but longer sequence.  The kernels of this file are instruction for instruction what they were when they shared
// gs_fused.hip with this call; dropping it is a change to device code, to be measured on its own (CHANGELOG.md).
size_t scan_counts_temp_bytes(size_t N) {
  size_t bytes = 0;
  (void)rocprim::exclusive_scan(nullptr, bytes, (int *)nullptr, (int *)nullptr, 0, N + 1, rocprim::plus<int>(), (hipStream_t)0);
  return bytes;
}

int launch_publish_counts(const int *rank_total, const int *offsets_total, const unsigned long long *pair_counters,
                          unsigned long long *pub, unsigned long long ticket, hipStream_t st) {
  publish_counts_kernel<<<1, 64, 0, st>>>(rank_total, offsets_total, pair_counters, pub, ticket);
  GS_LAUNCH_CHECK();
  return GSPLAT_OK;
}

}  // namespace gs
