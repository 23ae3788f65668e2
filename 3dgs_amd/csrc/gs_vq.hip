// gs_vq.hip -- vector quantisation of row vectors for the compressed scene export ("Compressed 3D Gaussian Splatting",
// Niedermayr et al. 2024; gsplat's PngCompression): gsplat_vq_assign finds every row's nearest centroid of a codebook,
// gsplat_vq_update moves every centroid to the mean of its rows; together one Lloyd iteration of k-means.  Definitions:
// include/gsplat_hip.h.
//
// gsplat_vq_assign is a GEMM whose output never leaves the registers: the score s[n,k] = |c_k|^2 - 2 x_n . c_k orders the
// centroids of row n as the squared distance does, and is formed on the f32-input matrix cores
// (v_mfma_f32_32x32x2_f32: bit for bit a k-ordered fmaf chain, 64 cycles per 32 x 32 x 2 product).
//   * Centroids are the A operand (the row index of the 32 x 32 result), points the B operand (the column index, which is
//     the lane): a lane holds 16 centroid scores of ITS point per product and keeps a running (min, index) in registers
//     across the whole codebook -- no cross-lane traffic until the two half-waves (k = lane >> 5, which hold rows 4h .. 4h+3
//     of every group of 8) are combined once at the end.
//   * The accumulator is initialised with |c_k|^2 and the centroids are staged in LDS as -2c, so the product IS the score.
//   * A wave owns 4 point tiles of 32 = 128 points whose coordinates stay in registers (one VGPR per k-step and tile, k
//     padded to even with zeros in registers), which gives 4 independent accumulators per centroid tile: the 64-cycle
//     dependent latency of the instruction is covered inside one wave.  A workgroup is 4 waves = 512 points.  The kernel is
//     instantiated for D <= 16, 32, 48 and 64 (the register array of the points is sized by it): up to 48 it fits 256
//     VGPRs and two workgroups share a CU, so that one wave's epilogue and staging run under the other's MFMAs.
//   * The codebook is streamed in stages of 64 centroids (128 in the D <= 64 form): fetched into registers while the
//     previous stage is multiplied, then written transposed into LDS ([d][centroid], pitch 33: writes and the operand
//     reads are conflict free) and its norms summed from there.  Per stage and workgroup that is 64 x D x 4 bytes against
//     2 x steps x 4 x 64 cycles of MFMA per wave: at D = 45, 11.5 KB per 11 776 cycles, and with two workgroups 2 bytes per
//     clock of the CU's 64.  The codebook (12 MB at K = 65 536, larger than an XCD's L2) is read once per 512 points: 23 GB
//     of L2 / fabric reads at N = 1e6 for 6.0e12 FLOP, 0.4 TB/s at the 60 ms the pass takes.
//   * After a 32-centroid tile the lane's 16 scores are reduced with min3 and the (min, index) scan runs only where the
//     tile holds a better score than the lane has: after a few thousand centroids that is rare.
//   * Every point scans the centroids in index order with a strict <, the half-waves are merged with the lower index
//     winning a tie: equal scores resolve to the lowest index, and two runs give the same bits.
// dist (optional) is a second, per-row kernel: the squared distance to the chosen centroid in double, rounded once.
//
// gsplat_vq_update: one group of 1 .. 64 lanes per (cluster, coordinate) walks the cluster's rows interleaved (lane g takes
// members g, g + G, ...), adds in double, the group is combined by a fixed butterfly and the mean rounded to float once.
// No atomics; an empty cluster is not written.
#include <cmath>

#include "gs_common.h"

namespace {

constexpr int kMaxD = 64, kMaxK = 65536;
constexpr int kThreads = 256, kWaves = kThreads / 64;
constexpr int kTiles = 4;                                                        // point tiles of 32 per wave
constexpr int kPointsPerWave = 32 * kTiles, kPointsPerBlock = kWaves * kPointsPerWave;  // 128, 512
constexpr int kPitch = 33;                                                       // floats per coordinate row of a 32-centroid tile

typedef float f32x16 __attribute__((ext_vector_type(16)));

struct AssignArgs {
  const float *x;   // [N, D]
  const float *cb;  // [K, D]
  int N, D, K;
  int *index;  // [N]
};

// kMaxSteps: the k-steps of 2 coordinates the registers are sized for (D <= 2 kMaxSteps); kBlocks: workgroups per CU;
// kStage: centroids per LDS stage
template <int kMaxSteps, int kBlocks, int kStage>
__global__ __launch_bounds__(kThreads, kBlocks) void vq_assign_kernel(AssignArgs a) {
  constexpr int kSub = kStage / 32;
  constexpr int kPre = kStage * 2 * kMaxSteps / kThreads;  // a thread's share of a stage, in floats
  __shared__ float s_c[kSub][2 * kMaxSteps * kPitch];  // -2c, [tile of 32 centroids][coordinate][centroid]
  __shared__ float s_norm[kStage];             // |c|^2, +inf past the codebook's end
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, j = lane & 31, h = lane >> 5;
  const int D = a.D, K = a.K, steps = (D + 1) >> 1;
  const long long p0 = (long long)blockIdx.x * kPointsPerBlock + wave * kPointsPerWave;

  // the coordinate rows D .. of the tiles are read by the last k-step of an odd D and never written: zero
  for (int e = tid; e < kSub * 2 * kMaxSteps * kPitch; e += kThreads) (&s_c[0][0])[e] = 0.f;

  // B operands: xr[s][t] = x[point j of tile t][coordinate 2s + h], zero past D and past N
  float xr[kMaxSteps][kTiles];
#pragma unroll
  for (int s = 0; s < kMaxSteps; ++s)
#pragma unroll
    for (int t = 0; t < kTiles; ++t) {
      const long long n = p0 + t * 32 + j;
      const int d = 2 * s + h;
      xr[s][t] = (n < a.N && d < D) ? a.x[(size_t)n * D + d] : 0.f;
    }

  float best[kTiles];
  int best_k[kTiles];
#pragma unroll
  for (int t = 0; t < kTiles; ++t) best[t] = INFINITY, best_k[t] = 0;

  // element e = r * kThreads + tid of a stage is coordinate d of centroid i: (i, d) of r = 0, and the step from r to r + 1
  const int i0 = tid / D, d0 = tid - i0 * D, qi = kThreads / D, qd = kThreads - qi * D;
  const int stages = (K + kStage - 1) / kStage;
  float pre[kPre];
  auto fetch = [&](int st) {
    const size_t base = (size_t)st * kStage * D;
    const int left = K - st * kStage, cnt = (left < kStage ? left : kStage) * D;
#pragma unroll
    for (int r = 0; r < kPre; ++r) {
      const int e = r * kThreads + tid;
      pre[r] = e < cnt ? a.cb[base + e] : 0.f;
    }
  };
  fetch(0);

  for (int st = 0; st < stages; ++st) {
    __syncthreads();  // the previous stage has been read (first trip: the tiles are zeroed)
    {
      int i = i0, d = d0;
#pragma unroll
      for (int r = 0; r < kPre; ++r) {
        if (r * kThreads + tid < kStage * D) s_c[i >> 5][d * kPitch + (i & 31)] = -2.f * pre[r];
        i += qi, d += qd;
        if (d >= D) d -= D, ++i;
      }
    }
    __syncthreads();
    if (tid < kStage) {
      const float *c = &s_c[tid >> 5][tid & 31];
      float s = 0.f;
#pragma unroll 8
      for (int d = 0; d < D; ++d) {
        const float v = c[d * kPitch];
        s = fmaf(v, v, s);
      }
      s_norm[tid] = st * kStage + tid < K ? 0.25f * s : INFINITY;
    }
    __syncthreads();
    if (st + 1 < stages) fetch(st + 1);  // in flight while this stage is multiplied

#pragma unroll 1
    for (int sub = 0; sub < kSub; ++sub) {
      const int k0 = st * kStage + sub * 32;
      if (k0 >= K) break;
      f32x16 acc[kTiles];
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const float nv = s_norm[sub * 32 + (r & 3) + 8 * (r >> 2) + 4 * h];
#pragma unroll
        for (int t = 0; t < kTiles; ++t) acc[t][r] = nv;
      }
      const float *cs = &s_c[sub][h * kPitch + j];  // A operand of k-step s: cs[2 s kPitch]
      float av = cs[0];
#pragma unroll
      for (int s = 0; s < kMaxSteps; ++s) {
        if (s < steps) {
          const float an = s + 1 < steps ? cs[2 * (s + 1) * kPitch] : 0.f;  // the next step's operand, behind this step's MFMAs
#pragma unroll
          for (int t = 0; t < kTiles; ++t) acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, xr[s][t], acc[t], 0, 0, 0);
          av = an;
        }
      }
      // The lane's 16 scores of a tile are reduced with min3 first: once a point has seen a few thousand centroids a tile
      // of 16 rarely holds a better one, and the scan below is skipped.  Register r is centroid row
      // (r & 3) + 8 (r >> 2) + 4 h: ascending in r, so the strict < (here and in the scan) keeps the lowest index.
#pragma unroll
      for (int t = 0; t < kTiles; ++t) {
        float m = acc[t][0];
#pragma unroll
        for (int r = 1; r < 16; r += 3) m = fminf(fminf(m, acc[t][r]), fminf(acc[t][r + 1], acc[t][r + 2]));
        if (m < best[t]) {
#pragma unroll
          for (int r = 0; r < 16; ++r)
            if (acc[t][r] < best[t]) best[t] = acc[t][r], best_k[t] = k0 + (r & 3) + 8 * (r >> 2) + 4 * h;
        }
      }
    }
  }

#pragma unroll
  for (int t = 0; t < kTiles; ++t) {
    const float ob = __shfl_xor(best[t], 32);
    const int ok = __shfl_xor(best_k[t], 32);
    if (ob < best[t] || (ob == best[t] && ok < best_k[t])) best_k[t] = ok;
    const long long n = p0 + t * 32 + j;
    if (h == 0 && n < a.N) a.index[n] = best_k[t];
  }
}

__global__ __launch_bounds__(256) void vq_dist_kernel(AssignArgs a, float *dist) {
  for (long long n = (long long)blockIdx.x * 256 + threadIdx.x; n < a.N; n += (long long)gridDim.x * 256) {
    const float *x = a.x + (size_t)n * a.D, *c = a.cb + (size_t)a.index[n] * a.D;
    double s = 0.0;
    for (int d = 0; d < a.D; ++d) {
      const double v = (double)x[d] - (double)c[d];
      s += v * v;
    }
    dist[n] = (float)s;
  }
}

struct UpdateArgs {
  const float *x;
  const int *order, *start;
  int D, K, lanes;
  float *cb;
};

__global__ __launch_bounds__(256) void vq_update_kernel(UpdateArgs a) {
  const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
  const long long item = t / a.lanes;  // (cluster, coordinate); the threads past the last item still take part in the butterfly
  const int g = (int)(t - item * a.lanes);
  const bool live = item < (long long)a.K * a.D;
  const int k = live ? (int)(item / a.D) : 0, d = live ? (int)(item - (long long)k * a.D) : 0;
  const int lo = live ? a.start[k] : 0, hi = live ? a.start[k + 1] : 0;
  double sum = 0.0;
  for (int m = lo + g; m < hi; m += a.lanes) sum += (double)a.x[(size_t)a.order[m] * a.D + d];
  for (int w = 1; w < a.lanes; w *= 2) sum += __shfl_xor(sum, w);
  if (live && g == 0 && hi > lo) a.cb[(size_t)k * a.D + d] = (float)(sum / (double)(hi - lo));
}

int check_sizes(const char *fn, int N, int D, int K) {
  GS_REQUIRE_IN(fn, D >= 1 && D <= kMaxD, "D must be 1 .. 64");
  GS_REQUIRE_IN(fn, K >= 1 && K <= kMaxK, "K must be 1 .. 65536");
  GS_REQUIRE_IN(fn, N >= 0, "N is negative");
  return GSPLAT_OK;
}

}  // namespace

extern "C" {

int gsplat_vq_assign(const float *x, const float *codebook, int N, int D, int K, int *index, float *dist, void *stream) {
  if (int rc = check_sizes(__func__, N, D, K)) return rc;
  if (N == 0) return GSPLAT_OK;
  GS_REQUIRE(x != nullptr && codebook != nullptr && index != nullptr, "x, codebook or index is null");
  GS_REQUIRE_DEV(x); GS_REQUIRE_DEV(codebook); GS_REQUIRE_DEV(index);
  if (dist) GS_REQUIRE_DEV(dist);
  hipStream_t st = (hipStream_t)stream;
  AssignArgs a = {x, codebook, N, D, K, index};
  const unsigned blocks = gs::div_up(N, kPointsPerBlock);
  if (D <= 16) vq_assign_kernel<8, 2, 64><<<blocks, kThreads, 0, st>>>(a);
  else if (D <= 32) vq_assign_kernel<16, 2, 64><<<blocks, kThreads, 0, st>>>(a);
  else if (D <= 48) vq_assign_kernel<24, 2, 64><<<blocks, kThreads, 0, st>>>(a);
  else vq_assign_kernel<32, 1, 128><<<blocks, kThreads, 0, st>>>(a);
  GS_LAUNCH_CHECK();
  if (dist) {
    vq_dist_kernel<<<(unsigned)std::min<long long>(8 * 1024, gs::div_up(N, 256)), 256, 0, st>>>(a, dist);
    GS_LAUNCH_CHECK();
  }
  return GSPLAT_OK;
}

int gsplat_vq_update(const float *x, const int *order, const int *start, int N, int D, int K, float *codebook,
                     void *stream) {
  if (int rc = check_sizes(__func__, N, D, K)) return rc;
  if (N == 0) return GSPLAT_OK;  // every cluster is empty
  GS_REQUIRE(x != nullptr && order != nullptr && start != nullptr && codebook != nullptr,
             "x, order, start or codebook is null");
  GS_REQUIRE_DEV(x); GS_REQUIRE_DEV(order); GS_REQUIRE_DEV(start); GS_REQUIRE_DEV(codebook);
  UpdateArgs a = {x, order, start, D, K, 1, codebook};
  // The group width comes from the MEAN cluster (the sizes are on the device, and reading the largest back would stall the
  // stream): 8 rows per lane at the mean.  A function of N and K alone, so the order of the additions is too.
  while (a.lanes < 64 && (long long)N > 8ll * a.lanes * K) a.lanes *= 2;
  vq_update_kernel<<<gs::div_up((long long)K * D * a.lanes, 256), 256, 0, (hipStream_t)stream>>>(a);
  GS_LAUNCH_CHECK();
  return GSPLAT_OK;
}

}  // extern "C"
