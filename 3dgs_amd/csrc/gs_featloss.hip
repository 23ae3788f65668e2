// gs_featloss.hip -- what trains a per-gaussian feature field: three losses on a feature map (gsplat_feature_ce_loss,
// gsplat_feature_l1_loss, gsplat_feature_cosine_loss) and the feature column's optimizer step
// (gsplat_feature_adam_step); definitions: include/gsplat_hip.h.
//
// A map is [rows, cols, C] float, channel-contiguous as gsplat_context_render_features writes it: a pixel's row is C
// consecutive floats.  One lane per pixel would read at a stride of 4 C bytes, so a pixel belongs to a sub-group of L lanes
// of one wave, L = 1, 4, 16 or 64 by C (shape_of below), and a lane holds at most kPieces x 4 elements of the row:
//   rows of whole 16-byte pieces (C % 4 == 0, every pointer 16-byte aligned): lane s holds pieces s, s + L, ... -- the L
//     lanes of a pixel, and the 64 / L pixels of a wave behind one another, read consecutive 16 bytes;
//   any other C: lane s holds elements s, s + L, s + 2 L, ... -- consecutive 4 bytes.
// The row stays in registers from the reductions (max, sums, dot products: an xor butterfly over the L lanes, the same
// tree in every run) to the gradient, so the map is read once at every C up to 512.  Like the other image-space
// regularisers (gs_regloss.h) everything is evaluated in double from the float maps -- the exponentials of the softmax
// are double exp of x - max -- and rounded to float once; the loss is summed in double per block and finished in a
// fixed order.  No atomics: two runs give the same bits.
#include <cmath>

#include "gs_common.h"
#include "gs_math.h"
#include "gs_regloss.h"

namespace {

constexpr int kMaxChannels = 512;
// as the normal map's losses (gs_normal.hip): more work per pixel than the depth regularisers, so up to eight blocks per
// CU; the scratch of the partial sums is sized for that
constexpr int kFeatBlocks = 8 * gs::kRegBlocks;

enum FeatureLoss { kCE = 0, kL1 = 1, kCosine = 2 };

struct FeatArgs {
  const float *map;            // [P, C]
  const float *target;         // [P, C]   (l1, cosine)
  const int *labels;           // [P]      (ce)
  const unsigned char *valid;  // [P] or null (l1, cosine)
  long long P;
  int C;
  double scale;    // weight / P (l1: weight / (P C))
  int add;         // the gradient is added to what grad holds
  float *grad;     // [P, C] or null
  double *partial; // the blocks' loss sums, or null
};

// the element of a row that slot (k, j) of lane s holds
template <int L, bool kVec>
__device__ __forceinline__ int elem_of(int s, int k, int j) {
  return kVec ? (k * L + s) * 4 + j : (k * 4 + j) * L + s;
}

// a lane's slots of the row at `row`; 0 where the row ends or when `on` is false (nothing is read then)
template <int L, int K, bool kVec>
__device__ __forceinline__ void load_row(const float *__restrict__ row, int C, int s, bool on, float (&v)[K][4]) {
#pragma unroll
  for (int k = 0; k < K; ++k) {
    if constexpr (kVec) {
      float4 q = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
      const int e = (k * L + s) * 4;
      if (on && e < C) q = *reinterpret_cast<const float4 *>(row + e);
      v[k][0] = q.x; v[k][1] = q.y; v[k][2] = q.z; v[k][3] = q.w;
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int e = (k * 4 + j) * L + s;
        v[k][j] = (on && e < C) ? row[e] : 0.0f;
      }
    }
  }
}

// a lane's slots of the gradient row: rounded to float once, stored or added (gs::put_grad's arithmetic)
template <int L, int K, bool kVec>
__device__ __forceinline__ void store_row(float *__restrict__ row, int C, int s, bool add, const double (&g)[K][4]) {
#pragma unroll
  for (int k = 0; k < K; ++k) {
    if constexpr (kVec) {
      const int e = (k * L + s) * 4;
      if (e < C) {
        float4 *dst = reinterpret_cast<float4 *>(row + e);
        float4 q = make_float4((float)g[k][0], (float)g[k][1], (float)g[k][2], (float)g[k][3]);
        if (add) {
          const float4 o = *dst;
          q.x = o.x + q.x; q.y = o.y + q.y; q.z = o.z + q.z; q.w = o.w + q.w;
        }
        *dst = q;
      }
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int e = (k * 4 + j) * L + s;
        if (e < C) {
          if (add) row[e] += (float)g[k][j];
          else row[e] = (float)g[k][j];
        }
      }
    }
  }
}

// the sum (the maximum) over the L lanes of a pixel, in every one of them: a fixed tree
template <int L>
__device__ __forceinline__ double group_sum(double v) {
#pragma unroll
  for (int off = L / 2; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}
template <int L>
__device__ __forceinline__ float group_max(float v) {
#pragma unroll
  for (int off = L / 2; off > 0; off >>= 1) v = fmaxf(v, __shfl_xor(v, off, 64));
  return v;
}

// 256 threads = 256 / L pixels per trip of a grid-stride loop.  Every lane of a block runs every trip to its end (the
// butterflies sit outside all per-pixel conditions); a pixel past the end or one that takes no part reads nothing.
template <int kLoss, int L, int K, bool kVec>
__global__ __launch_bounds__(256) void feature_loss_kernel(FeatArgs a) {
  constexpr int kPixels = 256 / L;
  const int tid = (int)threadIdx.x, s = tid % L, C = a.C;
  double sum = 0.0;
  for (long long base = (long long)blockIdx.x * kPixels; base < a.P; base += (long long)gridDim.x * kPixels) {
    const long long p = base + tid / L;
    const bool live = p < a.P;
    const size_t at = live ? (size_t)p * (size_t)C : 0;
    const float *row = a.map + at;
    float v[K][4];
    double g[K][4];
#pragma unroll
    for (int k = 0; k < K; ++k)
#pragma unroll
      for (int j = 0; j < 4; ++j) g[k][j] = 0.0;

    if constexpr (kLoss == kCE) {
      const int label = live ? a.labels[p] : -1;
      const bool part = label >= 0 && label < C;
      load_row<L, K, kVec>(row, C, s, part, v);
      float m = -INFINITY;
#pragma unroll
      for (int k = 0; k < K; ++k)
#pragma unroll
        for (int j = 0; j < 4; ++j)
          if (elem_of<L, kVec>(s, k, j) < C) m = fmaxf(m, v[k][j]);
      m = group_max<L>(m);
      double ex[K][4], z = 0.0;
#pragma unroll
      for (int k = 0; k < K; ++k)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          ex[k][j] = (part && elem_of<L, kVec>(s, k, j) < C) ? exp((double)v[k][j] - (double)m) : 0.0;
          z += ex[k][j];
        }
      z = group_sum<L>(z);
      if (part) {  // (z >= 1: the maximum's own term)
        const double inv = 1.0 / z;
#pragma unroll
        for (int k = 0; k < K; ++k)
#pragma unroll
          for (int j = 0; j < 4; ++j)
            g[k][j] = a.scale * (ex[k][j] * inv - (elem_of<L, kVec>(s, k, j) == label ? 1.0 : 0.0));
        if (s == 0) sum += (log(z) + (double)m) - (double)row[label];
      }
    } else {
      const bool part = live && (!a.valid || a.valid[p] != 0);
      float t[K][4];
      load_row<L, K, kVec>(row, C, s, part, v);
      load_row<L, K, kVec>(a.target + at, C, s, part, t);
      if constexpr (kLoss == kL1) {  // (slots past the row's end hold 0 - 0)
#pragma unroll
        for (int k = 0; k < K; ++k)
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const double d = (double)v[k][j] - (double)t[k][j];
            sum += fabs(d);
            g[k][j] = d > 0.0 ? a.scale : d < 0.0 ? -a.scale : 0.0;
          }
      } else {
        double dot = 0.0, ff = 0.0, tt = 0.0;
#pragma unroll
        for (int k = 0; k < K; ++k)
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const double f = (double)v[k][j], u = (double)t[k][j];
            dot += f * u; ff += f * f; tt += u * u;
          }
        dot = group_sum<L>(dot); ff = group_sum<L>(ff); tt = group_sum<L>(tt);
        if (part && ff > 0.0 && ff < HUGE_VAL && tt > 0.0 && tt < HUGE_VAL) {
          // d/df of 1 - f.t / (|f||t|) = -(t - (f.t / |f|^2) f) / (|f||t|)
          const double inv = 1.0 / (sqrt(ff) * sqrt(tt)), along = dot / ff;
#pragma unroll
          for (int k = 0; k < K; ++k)
#pragma unroll
            for (int j = 0; j < 4; ++j) g[k][j] = -a.scale * inv * ((double)t[k][j] - along * (double)v[k][j]);
          if (s == 0) sum += 1.0 - dot * inv;
        }
      }
    }
    if (a.grad && live) store_row<L, K, kVec>(a.grad + at, C, s, a.add != 0, g);
  }
  if (a.partial) gs::block_partial(sum, a.partial);
}

struct Shape { int lanes, pieces; };
// lanes per pixel and 16-byte (or 4 x 4-byte) pieces per lane: lanes x pieces x 4 >= C
Shape shape_of(int C) {
  if (C <= 4) return {1, 1};
  if (C <= 16) return {4, 1};
  if (C <= 64) return {16, 1};
  return {64, C <= 256 ? 1 : 2};
}

bool aligned16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

template <int kLoss, int L, int K>
void launch_shape(const FeatArgs &a, bool vec, int blocks, hipStream_t st) {
  if (vec) feature_loss_kernel<kLoss, L, K, true><<<blocks, 256, 0, st>>>(a);
  else feature_loss_kernel<kLoss, L, K, false><<<blocks, 256, 0, st>>>(a);
}

// the launch of one loss and, when its value is asked for, the finish of its partial sums
template <int kLoss>
int run_loss(FeatArgs a, float *loss_out, hipStream_t st) {
  const Shape sh = shape_of(a.C);
  const bool vec = a.C % 4 == 0 && aligned16(a.map) && aligned16(a.target) && aligned16(a.grad);
  const long long per_block = 256 / sh.lanes;
  const int blocks = (int)std::min<long long>(kFeatBlocks, (a.P + per_block - 1) / per_block);
  gs::ScratchLock lock;
  a.partial = nullptr;
  if (loss_out) {
    gs::DeviceBuffer &acc = gs::scratch(gs::SCR_DEPTH_LOSS);
    if (int rc = acc.reserve(kFeatBlocks * sizeof(double))) return rc;
    a.partial = acc.as<double>();
  }
  switch (sh.lanes * 4 + sh.pieces) {
    case 1 * 4 + 1: launch_shape<kLoss, 1, 1>(a, vec, blocks, st); break;
    case 4 * 4 + 1: launch_shape<kLoss, 4, 1>(a, vec, blocks, st); break;
    case 16 * 4 + 1: launch_shape<kLoss, 16, 1>(a, vec, blocks, st); break;
    case 64 * 4 + 1: launch_shape<kLoss, 64, 1>(a, vec, blocks, st); break;
    default: launch_shape<kLoss, 64, 2>(a, vec, blocks, st); break;
  }
  GS_LAUNCH_CHECK();
  if (loss_out) {
    gs::reg_loss_finish_kernel<<<1, 64, 0, st>>>(a.partial, blocks, a.scale, loss_out);
    GS_LAUNCH_CHECK();
  }
  return GSPLAT_OK;
}

// what the three losses refuse before anything else: sizes, the channel count, null pointers
int check_loss_args(const char *fn, const void *map, const void *second, int rows, int cols, int C, const float *grad_map,
                    const float *loss_out) {
  GS_REQUIRE_IN(fn, rows > 0 && cols > 0, "image size must be positive");
  GS_REQUIRE_IN(fn, C >= 1 && C <= kMaxChannels, "channels must be 1 .. 512");
  GS_REQUIRE_IN(fn, map != nullptr, "map is null");
  GS_REQUIRE_IN(fn, second != nullptr, "labels / target is null");
  GS_REQUIRE_IN(fn, grad_map != nullptr || loss_out != nullptr, "grad_map and loss_out are both null");
  GS_REQUIRE_DEV_IN(fn, map); GS_REQUIRE_DEV_IN(fn, second);
  if (grad_map) GS_REQUIRE_DEV_IN(fn, grad_map);
  if (loss_out) GS_REQUIRE_DEV_IN(fn, loss_out);
  return GSPLAT_OK;
}

// thread i owns element i of the [rows, C] index space of the rows the view saw, as optimizer_step_kernel (gs_loss.hip)
// does for a group of stride C; the element's step is gs::adam_values, the one that kernel applies
__global__ __launch_bounds__(256) void feature_adam_kernel(int rows, int C, const int *__restrict__ c2g,
                                                           float *__restrict__ param, float *__restrict__ exp_avg,
                                                           float *__restrict__ exp_avg_sq, float *__restrict__ grad,
                                                           float lr, float b1, float b2, float eps, float bias1,
                                                           float bias2) {
  const unsigned int i = blockIdx.x * 256u + threadIdx.x, stride = (unsigned int)C;
  if (i >= (unsigned int)rows * stride) return;
  const unsigned int r = i / stride, c = i - r * stride;
  const long long o = (long long)c2g[r] * stride + c;
  float pv = param[o], mv = exp_avg[o], vv = exp_avg_sq[o];
  gs::adam_values(pv, mv, vv, grad[o], lr, b1, b2, eps, bias1, bias2);
  param[o] = pv;
  exp_avg[o] = mv;
  exp_avg_sq[o] = vv;
  grad[o] = 0.0f;  // consumed: the accumulator is all zero again without a memset of its N x C floats
}

}  // namespace

extern "C" {

int gsplat_feature_ce_loss(const float *map, const int *labels, int rows, int cols, int channels, float weight,
                           int accumulate, float *grad_map, float *loss_out, void *stream) {
  if (int rc = check_loss_args(__func__, map, labels, rows, cols, channels, grad_map, loss_out)) return rc;
  FeatArgs a = {};
  a.map = map; a.labels = labels; a.P = (long long)rows * cols; a.C = channels;
  a.scale = (double)weight / (double)a.P; a.add = accumulate != 0; a.grad = grad_map;
  return run_loss<kCE>(a, loss_out, (hipStream_t)stream);
}

int gsplat_feature_l1_loss(const float *map, const float *target, const unsigned char *valid, int rows, int cols,
                           int channels, float weight, int accumulate, float *grad_map, float *loss_out, void *stream) {
  if (int rc = check_loss_args(__func__, map, target, rows, cols, channels, grad_map, loss_out)) return rc;
  if (valid) GS_REQUIRE_DEV(valid);
  FeatArgs a = {};
  a.map = map; a.target = target; a.valid = valid; a.P = (long long)rows * cols; a.C = channels;
  a.scale = (double)weight / ((double)a.P * (double)channels); a.add = accumulate != 0; a.grad = grad_map;
  return run_loss<kL1>(a, loss_out, (hipStream_t)stream);
}

int gsplat_feature_cosine_loss(const float *map, const float *target, const unsigned char *valid, int rows, int cols,
                               int channels, float weight, int accumulate, float *grad_map, float *loss_out,
                               void *stream) {
  if (int rc = check_loss_args(__func__, map, target, rows, cols, channels, grad_map, loss_out)) return rc;
  if (valid) GS_REQUIRE_DEV(valid);
  FeatArgs a = {};
  a.map = map; a.target = target; a.valid = valid; a.P = (long long)rows * cols; a.C = channels;
  a.scale = (double)weight / (double)a.P; a.add = accumulate != 0; a.grad = grad_map;
  return run_loss<kCosine>(a, loss_out, (hipStream_t)stream);
}

int gsplat_feature_adam_step(const int *compact_to_global, int num_culled, int channels, float *features, float *exp_avg,
                             float *exp_avg_sq, float *grad_global, float lr, float b1, float b2, float eps, float bias1,
                             float bias2, void *stream) {
  GS_REQUIRE(num_culled >= 0, "negative gaussian count");
  GS_REQUIRE(channels >= 1 && channels <= kMaxChannels, "channels must be 1 .. 512");
  if (num_culled == 0) return GSPLAT_OK;
  GS_REQUIRE(compact_to_global && features && exp_avg && exp_avg_sq && grad_global, "a required pointer is null");
  GS_REQUIRE_DEV(compact_to_global); GS_REQUIRE_DEV(features); GS_REQUIRE_DEV(exp_avg); GS_REQUIRE_DEV(exp_avg_sq);
  GS_REQUIRE_DEV(grad_global);
  const long long n = (long long)num_culled * channels;
  GS_REQUIRE(n < (1ll << 31), "too many parameters for one launch");
  feature_adam_kernel<<<gs::div_up(n, 256), 256, 0, (hipStream_t)stream>>>(num_culled, channels, compact_to_global,
                                                                           features, exp_avg, exp_avg_sq, grad_global, lr,
                                                                           b1, b2, eps, bias1, bias2);
  GS_LAUNCH_CHECK();
  return GSPLAT_OK;
}

}  // extern "C"
