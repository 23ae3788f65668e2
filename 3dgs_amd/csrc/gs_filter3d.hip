// gs_filter3d.hip -- the 3D smoothing filter of Mip-Splatting (Yu et al., CVPR 2024, section 4.1): every gaussian is
// band-limited to the sampling rate of the training cameras that see it.  The 2D half of that paper is the context's
// anti-aliased mode (gs_math.h: conic_radius<true>); this file is the 3D half.
//
//   filter3d[i] = sqrt(0.2) * min over the cameras k that sample gaussian i of  z_k / focal_x_k
// is the standard deviation of the low-pass gaussian (0.2 = the paper's s), and the gaussian enters the rasterizer as
//   Sigma_eff = Sigma + f^2 I   (R orthonormal: scale_eff_k = 1/2 log(exp(2 scale_k) + f^2))
//   o         = sigmoid(opacity) * sqrt(det Sigma / det Sigma_eff)
// The filter does not depend on the camera a view is rendered from, so it is a parameter transform in front of the
// forward (filter3d_apply) and a chain rule behind the per-gaussian backward (filter3d_apply_backward): the compositing
// and per-gaussian kernels see ordinary parameters (gsplat_context_set_filter3d: gs_context.hip; the calls: gs_fused.hip).
// Everything is one thread per gaussian.
#include "gs_common.h"
#include "gs_launch.h"
#include "gs_math.h"

namespace {

constexpr int kBlock = 256;
constexpr int kCamChunk = 32;  // cameras staged in LDS at a time: 32 x (12 + 16 + 1 floats, 2 ints) = 3968 bytes

// Per camera chunk: rows 0..2 of the view, the projection, focal_x, and (width, height).  Every lane of a wave reads the
// same LDS address at the same time (a broadcast).
struct CamChunk {
  float view[kCamChunk][12];
  float proj[kCamChunk][16];
  float focal[kCamChunk];
  int size[kCamChunk][2];
};

// t_out[i] = min over the cameras that sample gaussian i of z / focal_x, or -1 when none does; *max_bits = the bits of the
// largest such minimum (integer atomicMax on the bits of non-negative floats: the same value whatever the order).
// Camera k samples a gaussian when it lies in front of the near plane and within 15 % of the image's size around the
// image -- (u, v) are the pixel coordinates the forward computes (gs::camera_space, gs::to_screen).
__global__ __launch_bounds__(kBlock) void filter3d_min_kernel(const float *__restrict__ xyz, int N,
                                                              const float *__restrict__ views,
                                                              const float *__restrict__ projs,
                                                              const float *__restrict__ focal_x,
                                                              const int *__restrict__ sizes, int V, float near_thresh,
                                                              float *__restrict__ t_out,
                                                              unsigned int *__restrict__ max_bits) {
  __shared__ CamChunk s;
  const int i = blockIdx.x * kBlock + threadIdx.x;
  const bool live = i < N;
  float wx = 0.0f, wy = 0.0f, wz = 0.0f;
  if (live) { wx = xyz[3 * (size_t)i]; wy = xyz[3 * (size_t)i + 1]; wz = xyz[3 * (size_t)i + 2]; }
  float t = -1.0f;
  for (int c0 = 0; c0 < V; c0 += kCamChunk) {
    const int n = min(kCamChunk, V - c0);
    if (c0 > 0) __syncthreads();  // the chunk before has been read by every wave
    for (int e = threadIdx.x; e < n * 16; e += kBlock) {
      const int cam = e >> 4, k = e & 15;
      const size_t src = (size_t)(c0 + cam) * 16 + k;
      if (k < 12) s.view[cam][k] = views[src];
      s.proj[cam][k] = projs[src];
      if (k == 12) s.focal[cam] = focal_x[c0 + cam];
      if (k >= 14) s.size[cam][k - 14] = sizes[2 * (size_t)(c0 + cam) + (k - 14)];
    }
    __syncthreads();
    if (!live) continue;
    for (int cam = 0; cam < n; ++cam) {
      const gs::Mat34 vw = gs::load_view(s.view[cam]);
      const gs::Mat44 pr = gs::load_proj(s.proj[cam]);
      const int W = s.size[cam][0], H = s.size[cam][1];
      float x, y, z, u, v;
      gs::camera_space(vw, wx, wy, wz, x, y, z);
      gs::to_screen(pr, x, y, z, W, H, u, v);
      const float fw = (float)W, fh = (float)H;
      const bool sampled = z > near_thresh && u >= -0.15f * fw && u <= 1.15f * fw && v >= -0.15f * fh && v <= 1.15f * fh;
      if (sampled) {
        const float tk = z / s.focal[cam];
        if (tk >= 0.0f && (t < 0.0f || tk < t)) t = tk;  // (a NaN or negative ratio -- a focal length <= 0 -- samples nothing)
      }
    }
  }
  if (live) t_out[i] = t;
  unsigned int m = t >= 0.0f ? __float_as_uint(t) : 0u;  // non-negative floats order like their bits
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) m = max(m, (unsigned int)__shfl_xor((int)m, off, 64));
  if ((threadIdx.x & 63) == 0 && m != 0u) atomicMax(max_bits, m);
}

// rows no camera samples take the largest t of the sampled ones (0 when there is none); t -> sqrt(0.2) t
__global__ __launch_bounds__(kBlock) void filter3d_fill_kernel(int N, const unsigned int *__restrict__ max_bits,
                                                               float *__restrict__ filter3d) {
  const int i = blockIdx.x * kBlock + threadIdx.x;
  if (i >= N) return;
  float t = filter3d[i];
  if (!(t >= 0.0f)) t = __uint_as_float(*max_bits);
  filter3d[i] = sqrtf(0.2f) * t;
}

// One axis.  With a = 2 (scale - log f), i.e. e^a = s^2 / f^2, and e = exp(-|a|) in (0, 1]:
//   scale_eff = max(scale, log f) + 1/2 log(1 + e)          (= 1/2 log(s^2 + f^2); neither term overflows)
//   d  = scale - scale_eff  (<= 0: the axis' share of log rho3)
//   w  = s^2 / (s^2 + f^2) = d scale_eff / d scale,   wc = 1 - w, each formed without cancellation
__device__ __forceinline__ void filter3d_axis(float sc, float lf, float &eff, float &d, float &w, float &wc) {
  const float a = 2.0f * (sc - lf);
  const float e = expf(-fabsf(a));
  const float h = 0.5f * log1pf(e);
  const float r = 1.0f / (1.0f + e);
  if (a >= 0.0f) { eff = sc + h; d = -h; w = r; wc = e * r; }
  else { eff = lf + h; d = (sc - lf) - h; w = e * r; wc = r; }
}

// log o = log sigmoid(x) + log rho3 and 1 - o = -expm1(log o): exact where sigmoid(x) rho3 rounds to 1
__device__ __forceinline__ float filter3d_log_o(float x, float dsum) {
  const float ls = x >= 0.0f ? -log1pf(expf(-x)) : x - log1pf(expf(x));
  return ls + dsum;
}

// (scale, opacity) -> (scale_eff, logit(sigmoid(opacity) rho3)); a row with f == 0 (or a NaN / negative f: no filter)
// passes through with its bits unchanged
__global__ __launch_bounds__(kBlock) void filter3d_apply_kernel(const float *__restrict__ scale,
                                                                const float *__restrict__ opacity,
                                                                const float *__restrict__ filter3d, int N,
                                                                float *__restrict__ scale_eff,
                                                                float *__restrict__ opacity_eff) {
  const int i = blockIdx.x * kBlock + threadIdx.x;
  if (i >= N) return;
  const float f = filter3d[i], x = opacity[i];
  const float s0 = scale[3 * (size_t)i], s1 = scale[3 * (size_t)i + 1], s2 = scale[3 * (size_t)i + 2];
  float e0 = s0, e1 = s1, e2 = s2, xo = x;
  if (f > 0.0f) {
    const float lf = logf(f);
    float d0, d1, d2, w, wc;
    filter3d_axis(s0, lf, e0, d0, w, wc);
    filter3d_axis(s1, lf, e1, d1, w, wc);
    filter3d_axis(s2, lf, e2, d2, w, wc);
    const float lo = filter3d_log_o(x, (d0 + d1) + d2);
    const float om = -expm1f(lo);
    if (om > 0.0f) xo = lo - logf(om);  // (o == 1 in float: the filter changes nothing the logit can express)
  }
  scale_eff[3 * (size_t)i] = e0; scale_eff[3 * (size_t)i + 1] = e1; scale_eff[3 * (size_t)i + 2] = e2;
  opacity_eff[i] = xo;
}

// The chain rule, in place on stored gradients g_s (with respect to scale_eff) and g_o (with respect to opacity_eff):
//   k = g_o / (1 - o) (0 where 1 - o == 0: gs::effective_opacity_bwd's convention)
//   grad_scale_k = g_s_k w_k + k (1 - w_k),   grad_opacity = k (1 - sigmoid(opacity))
// Gradient row j belongs to gaussian rows[j] (NULL: j) and lies at grad_scale + r * scale_stride, grad_opacity + r *
// opacity_stride with r = j, or r = the gaussian's index when `at_gaussian` (rows of a global-order array).  first < end:
// only the rows whose gaussian lies in [first, end); `rows` is then increasing (compact_to_global) and the grid covers
// the range's largest possible number of slots from the first one.
__global__ __launch_bounds__(kBlock) void filter3d_apply_bwd_kernel(const float *__restrict__ scale,
                                                                    const float *__restrict__ opacity,
                                                                    const float *__restrict__ filter3d,
                                                                    const int *__restrict__ rows, int M,
                                                                    float *__restrict__ grad_scale, int scale_stride,
                                                                    float *__restrict__ grad_opacity,
                                                                    int opacity_stride, int at_gaussian, int first,
                                                                    int end) {
  int j = blockIdx.x * kBlock + threadIdx.x;
  if (first < end) {  // lower bound of `first` in rows[0..M): the same for every thread
    int lo = 0, hi = M;
    while (lo < hi) {
      const int mid = lo + ((hi - lo) >> 1);
      if (rows[mid] < first) lo = mid + 1; else hi = mid;
    }
    j += lo;
  }
  if (j >= M) return;
  const int i = rows ? rows[j] : j;
  if (first < end && i >= end) return;
  const float f = filter3d[i];
  if (!(f > 0.0f)) return;
  const size_t r = at_gaussian ? (size_t)i : (size_t)j;
  float *gs_row = grad_scale + r * (size_t)scale_stride, *go_row = grad_opacity + r * (size_t)opacity_stride;
  const float x = opacity[i], lf = logf(f);
  float eff, d[3], w[3], wc[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) filter3d_axis(scale[3 * (size_t)i + k], lf, eff, d[k], w[k], wc[k]);
  const float om = -expm1f(filter3d_log_o(x, (d[0] + d[1]) + d[2]));
  const float g_o = *go_row;
  const float kq = om == 0.0f ? 0.0f : g_o / om;
  const float ex = expf(-fabsf(x));
  const float one_minus_sig = x >= 0.0f ? ex / (1.0f + ex) : 1.0f / (1.0f + ex);
#pragma unroll
  for (int k = 0; k < 3; ++k) gs_row[k] = gs_row[k] * w[k] + kq * wc[k];
  *go_row = kq * one_minus_sig;
}

}  // namespace

namespace gs {

int launch_filter3d_apply(const float *scale, const float *opacity, const float *filter3d, int N, float *scale_eff,
                          float *opacity_eff, hipStream_t st) {
  if (N == 0) return GSPLAT_OK;
  filter3d_apply_kernel<<<div_up(N, kBlock), kBlock, 0, st>>>(scale, opacity, filter3d, N, scale_eff, opacity_eff);
  GS_LAUNCH_CHECK();
  return GSPLAT_OK;
}

// `span`: the number of slots the grid has to cover (M, or for a range at most end - first)
int launch_filter3d_apply_bwd(const float *scale, const float *opacity, const float *filter3d, const int *rows, int M,
                              float *grad_scale, int scale_stride, float *grad_opacity, int opacity_stride,
                              bool at_gaussian, int first, int end, int span, hipStream_t st) {
  if (span <= 0) return GSPLAT_OK;
  filter3d_apply_bwd_kernel<<<div_up(span, kBlock), kBlock, 0, st>>>(scale, opacity, filter3d, rows, M, grad_scale,
                                                                     scale_stride, grad_opacity, opacity_stride,
                                                                     at_gaussian ? 1 : 0, first, end);
  GS_LAUNCH_CHECK();
  return GSPLAT_OK;
}

}  // namespace gs

extern "C" {

int gsplat_compute_filter3d(const float *xyz, int N, const float *views, const float *projs, const float *focal_x,
                            const int *sizes, int V, float near_thresh, float *filter3d, void *stream) {
  GS_REQUIRE(N >= 0 && V > 0, "N must not be negative and there must be a camera");
  GS_REQUIRE(near_thresh >= 0.0f, "near must not be negative");  // (the maximum is taken on the bits of non-negative floats)
  if (N == 0) return GSPLAT_OK;
  GS_REQUIRE_DEV(xyz); GS_REQUIRE_DEV(views); GS_REQUIRE_DEV(projs); GS_REQUIRE_DEV(focal_x); GS_REQUIRE_DEV(sizes);
  GS_REQUIRE_DEV(filter3d);
  hipStream_t st = (hipStream_t)stream;
  // the cell of the maximum: a pool block, handed back in stream order (the next user queues behind the fill kernel)
  void *cell = nullptr;
  int rc = gsplat_pool_alloc_on(&cell, sizeof(unsigned int), stream);
  if (rc) return rc;
  hipError_t e = hipMemsetAsync(cell, 0, sizeof(unsigned int), st);
  if (e == hipSuccess) {
    filter3d_min_kernel<<<gs::div_up(N, kBlock), kBlock, 0, st>>>(xyz, N, views, projs, focal_x, sizes, V, near_thresh,
                                                                  filter3d, (unsigned int *)cell);
    filter3d_fill_kernel<<<gs::div_up(N, kBlock), kBlock, 0, st>>>(N, (const unsigned int *)cell, filter3d);
    e = hipGetLastError();
  }
  rc = gsplat_pool_free_on(cell, stream);
  if (e != hipSuccess) {
    gs::set_error("gsplat_compute_filter3d: %s", hipGetErrorString(e));
    return GSPLAT_ERR_HIP;
  }
  return rc;
}

int gsplat_filter3d_apply(const float *scale, const float *opacity, const float *filter3d, int N, float *scale_eff,
                          float *opacity_eff, void *stream) {
  GS_REQUIRE(N >= 0, "N must not be negative");
  if (N == 0) return GSPLAT_OK;
  GS_REQUIRE_DEV(scale); GS_REQUIRE_DEV(opacity); GS_REQUIRE_DEV(filter3d); GS_REQUIRE_DEV(scale_eff);
  GS_REQUIRE_DEV(opacity_eff);
  return gs::launch_filter3d_apply(scale, opacity, filter3d, N, scale_eff, opacity_eff, (hipStream_t)stream);
}

int gsplat_filter3d_apply_backward(const float *scale, const float *opacity, const float *filter3d, const int *rows,
                                   int M, float *grad_scale, int scale_stride, float *grad_opacity, int opacity_stride,
                                   void *stream) {
  GS_REQUIRE(M >= 0, "M must not be negative");
  GS_REQUIRE(scale_stride >= 3 && opacity_stride >= 1, "a gradient row holds three scale gradients and one opacity gradient");
  if (M == 0) return GSPLAT_OK;
  GS_REQUIRE_DEV(scale); GS_REQUIRE_DEV(opacity); GS_REQUIRE_DEV(filter3d); GS_REQUIRE_DEV(grad_scale);
  GS_REQUIRE_DEV(grad_opacity);
  if (rows) GS_REQUIRE_DEV(rows);
  return gs::launch_filter3d_apply_bwd(scale, opacity, filter3d, rows, M, grad_scale, scale_stride, grad_opacity,
                                       opacity_stride, false, 0, 0, M, (hipStream_t)stream);
}

}  // extern "C"
