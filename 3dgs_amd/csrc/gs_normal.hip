// gs_normal.hip -- normal maps from the rendered depth (gsplat_depth_to_normal, gsplat_depth_to_normal_backward) and the
// two losses on them (gsplat_normal_prior_loss, gsplat_normal_smoothness_loss); definitions: include/gsplat_hip.h.
//
// Like the depth regularisers of gs_loss.hip, every pixel is evaluated in double from the float maps and rounded to float
// once, and a loss is summed in double per block and finished in a fixed order (gs_regloss.h).  Every kernel GATHERS: a
// thread owns an output pixel and reads what it needs, nothing is added with atomics, two runs give the same bits.
//
// The two stencils run on 64 x 16 pixel tiles: 256 threads as four rows of one 64-lane wave each (a wave's loads and
// stores are one contiguous run of a map's row), a thread takes rows ty, ty + 4, ty + 8, ty + 12 of its column.  The
// expected depth z of the tile plus its halo (1 pixel forward, 2 backward: a pixel's gradient comes from its four
// neighbours' normals, which read THEIR four neighbours) is staged in LDS as doubles, so depth and T are read once per
// block; z = 0 stands for "not ok" and for "outside the image" alike (an ok pixel has z > 0), which makes the one-pixel
// border invalid without a test of its own.  The backward recomputes its neighbours' cross products from the staged z
// and reads nothing of the normal map.
#include <cmath>

#include "gs_common.h"
#include "gs_regloss.h"

namespace {

using gs::block_partial;
using gs::put_grad;

constexpr int kNW = 64, kNH = 16, kNRows = 4;  // tile width, tile height, thread rows
static_assert(kNW * kNRows == 256 && kNH % kNRows == 0, "tile shape vs 256 threads");

struct Intrinsics { double fx, fy, cx, cy; };

// z of an ok pixel (A >= alpha_min, depth > 0, both finite), 0 otherwise
__device__ __forceinline__ double expected_depth(float depth, float T, int inverse, double alpha_min) {
  const double A = 1.0 - (double)T, d = (double)depth;
  const bool ok = A >= alpha_min && A < HUGE_VAL && d > 0.0 && d < HUGE_VAL;
  if (!ok) return 0.0;
  return inverse ? A / d : d / A;
}

// the tile at (x0, y0) plus R pixels all round -> s[(kNH + 2R)][(kNW + 2R)]
template <int R>
__device__ __forceinline__ void stage_depth(double *__restrict__ s, const float *__restrict__ depth,
                                            const float *__restrict__ T, int H, int W, int x0, int y0, int inverse,
                                            double alpha_min, int tid) {
  constexpr int SW = kNW + 2 * R, SH = kNH + 2 * R;
  for (int e = tid; e < SW * SH; e += 256) {
    const int ly = e / SW, lx = e - ly * SW;
    const int gx = x0 + lx - R, gy = y0 + ly - R;
    double z = 0.0;
    if (gx >= 0 && gx < W && gy >= 0 && gy < H) {
      const size_t i = (size_t)gy * W + gx;
      z = expected_depth(depth[i], T[i], inverse, alpha_min);
    }
    s[e] = z;
  }
}

// c = ty x tx of the pixel at s[0] (pitch: doubles per staged row) with the ray coordinates rx[0..2] of columns x - 1, x,
// x + 1 and ry[0..2] of rows y - 1, y, y + 1.  False when the pixel or one of its four neighbours is not ok.
__device__ __forceinline__ bool normal_cross(const double *__restrict__ s, int pitch, const double *rx, const double *ry,
                                             double (&tx)[3], double (&ty)[3], double (&c)[3]) {
  const double zc = s[0], zl = s[-1], zr = s[1], zu = s[-pitch], zd = s[pitch];
  if (zc == 0.0 || zl == 0.0 || zr == 0.0 || zu == 0.0 || zd == 0.0) return false;
  tx[0] = zr * rx[2] - zl * rx[0]; tx[1] = zr * ry[1] - zl * ry[1]; tx[2] = zr - zl;
  ty[0] = zd * rx[1] - zu * rx[1]; ty[1] = zd * ry[2] - zu * ry[0]; ty[2] = zd - zu;
  c[0] = ty[1] * tx[2] - ty[2] * tx[1];
  c[1] = ty[2] * tx[0] - ty[0] * tx[2];
  c[2] = ty[0] * tx[1] - ty[1] * tx[0];
  return true;
}

__global__ __launch_bounds__(256) void depth_to_normal_kernel(const float *__restrict__ depth, const float *__restrict__ T,
                                                              int H, int W, Intrinsics k, int inverse, double alpha_min,
                                                              float *__restrict__ normal) {
  constexpr int R = 1, SW = kNW + 2 * R;
  __shared__ double s_z[SW * (kNH + 2 * R)];
  const int x0 = blockIdx.x * kNW, y0 = blockIdx.y * kNH;
  stage_depth<R>(s_z, depth, T, H, W, x0, y0, inverse, alpha_min, (int)(threadIdx.y * kNW + threadIdx.x));
  __syncthreads();
  const int x = x0 + (int)threadIdx.x;
  if (x >= W) return;
  double rx[3];
#pragma unroll
  for (int j = 0; j < 3; ++j) rx[j] = ((double)(x - 1 + j) - k.cx) / k.fx;
  for (int ly = threadIdx.y; ly < kNH; ly += kNRows) {
    const int y = y0 + ly;
    if (y >= H) break;
    double ry[3], tx[3], ty[3], c[3], n[3] = {0.0, 0.0, 0.0};
#pragma unroll
    for (int j = 0; j < 3; ++j) ry[j] = ((double)(y - 1 + j) - k.cy) / k.fy;
    if (normal_cross(&s_z[(ly + R) * SW + (int)threadIdx.x + R], SW, rx, ry, tx, ty, c)) {
      const double len = sqrt(c[0] * c[0] + c[1] * c[1] + c[2] * c[2]);
      if (len > 0.0 && len < HUGE_VAL) { n[0] = c[0] / len; n[1] = c[1] / len; n[2] = c[2] / len; }
    }
    float *o = normal + ((size_t)y * W + x) * 3;
    o[0] = (float)n[0]; o[1] = (float)n[1]; o[2] = (float)n[2];
  }
}

// What the normal at the staged position s (pixel p, whose gradient G = dL/dn is g[0..2]) sends to ONE END of its tx
// (kAlongX) or ty, as the dot product with that end's ray `rq`: with gc = dL/dc = (G - n (n . G)) / |c|,
// dL/dtx = gc x ty and dL/dty = tx x gc.  0 when p has no normal.
template <bool kAlongX>
__device__ __forceinline__ double tangent_gradient(const double *__restrict__ s, int pitch, const double *rx,
                                                   const double *ry, const float *__restrict__ g, const double (&rq)[3]) {
  double tx[3], ty[3], c[3];
  if (!normal_cross(s, pitch, rx, ry, tx, ty, c)) return 0.0;
  const double len = sqrt(c[0] * c[0] + c[1] * c[1] + c[2] * c[2]);
  if (!(len > 0.0 && len < HUGE_VAL)) return 0.0;
  const double inv = 1.0 / len;  // (one division for the six by |c|: a pixel pays for four of these)
  const double n[3] = {c[0] * inv, c[1] * inv, c[2] * inv};
  const double G[3] = {(double)g[0], (double)g[1], (double)g[2]};
  const double nG = n[0] * G[0] + n[1] * G[1] + n[2] * G[2];
  const double gc[3] = {(G[0] - n[0] * nG) * inv, (G[1] - n[1] * nG) * inv, (G[2] - n[2] * nG) * inv};
  double d[3];
  if constexpr (kAlongX) {  // gc x ty
    d[0] = gc[1] * ty[2] - gc[2] * ty[1]; d[1] = gc[2] * ty[0] - gc[0] * ty[2]; d[2] = gc[0] * ty[1] - gc[1] * ty[0];
  } else {                  // tx x gc
    d[0] = tx[1] * gc[2] - tx[2] * gc[1]; d[1] = tx[2] * gc[0] - tx[0] * gc[2]; d[2] = tx[0] * gc[1] - tx[1] * gc[0];
  }
  return d[0] * rq[0] + d[1] * rq[1] + d[2] * rq[2];
}

template <bool kAdd>
__global__ __launch_bounds__(256) void depth_to_normal_backward_kernel(const float *__restrict__ depth,
                                                                       const float *__restrict__ T, int H, int W,
                                                                       Intrinsics k, int inverse, double alpha_min,
                                                                       const float *__restrict__ grad_normal,
                                                                       float *__restrict__ grad_depth,
                                                                       float *__restrict__ grad_alpha) {
  constexpr int R = 2, SW = kNW + 2 * R;
  __shared__ double s_z[SW * (kNH + 2 * R)];
  const int x0 = blockIdx.x * kNW, y0 = blockIdx.y * kNH;
  stage_depth<R>(s_z, depth, T, H, W, x0, y0, inverse, alpha_min, (int)(threadIdx.y * kNW + threadIdx.x));
  __syncthreads();
  const int x = x0 + (int)threadIdx.x;
  if (x >= W) return;
  double rx[5];  // columns x - 2 .. x + 2
#pragma unroll
  for (int j = 0; j < 5; ++j) rx[j] = ((double)(x - 2 + j) - k.cx) / k.fx;
  for (int ly = threadIdx.y; ly < kNH; ly += kNRows) {
    const int y = y0 + ly;
    if (y >= H) break;
    const size_t i = (size_t)y * W + x;
    const double *s = &s_z[(ly + R) * SW + (int)threadIdx.x + R];
    const double zq = s[0];
    double g_depth = 0.0, g_alpha = 0.0;
    if (zq != 0.0) {  // (a pixel that is not ok enters no valid normal; a neighbour with z != 0 lies inside the image)
      double ry[5];
#pragma unroll
      for (int j = 0; j < 5; ++j) ry[j] = ((double)(y - 2 + j) - k.cy) / k.fy;
      const double rq[3] = {rx[2], ry[2], 1.0};
      const float *G = grad_normal + i * 3;
      double dz = 0.0;
      // this pixel is the right end of its left neighbour's tx, the left end of its right neighbour's, the lower end of
      // its upper neighbour's ty and the upper end of its lower neighbour's
      if (s[-1] != 0.0) dz += tangent_gradient<true>(s - 1, SW, rx, ry + 1, G - 3, rq);
      if (s[1] != 0.0) dz -= tangent_gradient<true>(s + 1, SW, rx + 2, ry + 1, G + 3, rq);
      if (s[-SW] != 0.0) dz += tangent_gradient<false>(s - SW, SW, rx + 1, ry, G - (size_t)W * 3, rq);
      if (s[SW] != 0.0) dz -= tangent_gradient<false>(s + SW, SW, rx + 1, ry + 2, G + (size_t)W * 3, rq);
      const double d = (double)depth[i], A = 1.0 - (double)T[i];
      if (inverse) { g_depth = dz * (-zq / d); g_alpha = dz * (1.0 / d); }   // z = A / depth
      else { g_depth = dz * (1.0 / A); g_alpha = dz * (-zq / A); }           // z = depth / A
    }
    put_grad<kAdd>(grad_depth, (long long)i, g_depth);
    put_grad<kAdd>(grad_alpha, (long long)i, g_alpha);
  }
}

__device__ __forceinline__ bool has_normal(const float *__restrict__ n) { return n[0] != 0.0f || n[1] != 0.0f || n[2] != 0.0f; }

// 1 - n . prior / |prior| over the pixels with a normal and a non-zero prior; `scale` = weight / P
template <bool kAdd>
__global__ __launch_bounds__(256) void normal_prior_loss_kernel(long long n, const float *__restrict__ normal,
                                                                const float *__restrict__ prior, double scale,
                                                                float *__restrict__ grad_normal,
                                                                double *__restrict__ partial) {
  double sum = 0.0;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
    const float *nn = normal + i * 3, *pp = prior + i * 3;
    const double p[3] = {(double)pp[0], (double)pp[1], (double)pp[2]};
    const double len = sqrt(p[0] * p[0] + p[1] * p[1] + p[2] * p[2]);
    double g[3] = {0.0, 0.0, 0.0};
    if (has_normal(nn) && len > 0.0 && len < HUGE_VAL) {
      const double u[3] = {p[0] / len, p[1] / len, p[2] / len};
      sum += 1.0 - ((double)nn[0] * u[0] + (double)nn[1] * u[1] + (double)nn[2] * u[2]);
      g[0] = -scale * u[0]; g[1] = -scale * u[1]; g[2] = -scale * u[2];
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) put_grad<kAdd>(grad_normal, i * 3 + c, g[c]);
  }
  if (partial) block_partial(sum, partial);
}

// w_ab sum_c |n_a,c - n_b,c| over the adjacent pairs of pixels with a normal.  The thread of pixel a gathers its (up to)
// four pairs for the gradient, and counts the pairs with its right and lower neighbour for the loss (every pair once).
template <bool kAdd>
__global__ __launch_bounds__(256) void normal_smoothness_loss_kernel(int H, int W, const float *__restrict__ normal,
                                                                     const float *__restrict__ image, double edge_scale,
                                                                     double scale, float *__restrict__ grad_normal,
                                                                     double *__restrict__ partial) {
  const long long n = (long long)H * W;
  double sum = 0.0;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
    const int y = (int)(i / W), x = (int)(i - (long long)y * W);
    const float *na = normal + i * 3;
    double g[3] = {0.0, 0.0, 0.0};
    if (has_normal(na)) {
      const double a[3] = {(double)na[0], (double)na[1], (double)na[2]};
#pragma unroll
      for (int dir = 0; dir < 4; ++dir) {  // right, down (counted for the loss), left, up
        const int bx = x + (dir == 0) - (dir == 2), by = y + (dir == 1) - (dir == 3);
        if (bx < 0 || bx >= W || by < 0 || by >= H) continue;
        const long long j = (long long)by * W + bx;
        const float *nb = normal + j * 3;
        if (!has_normal(nb)) continue;
        double w = 1.0;
        if (image) {
          const float *ia = image + i * 3, *ib = image + j * 3;
          const double diff = fabs((double)ia[0] - (double)ib[0]) + fabs((double)ia[1] - (double)ib[1]) +
                              fabs((double)ia[2] - (double)ib[2]);
          w = exp(-edge_scale * (diff / 3.0));
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          const double d = a[c] - (double)nb[c];
          g[c] += d > 0.0 ? w : d < 0.0 ? -w : 0.0;
          if (dir < 2) sum += w * fabs(d);
        }
      }
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) put_grad<kAdd>(grad_normal, i * 3 + c, scale * g[c]);
  }
  if (partial) block_partial(sum, partial);
}

// the checks the two stencils share; `fn`: the public function that was called
int check_stencil_args(const char *fn, const float *depth, const float *T, int rows, int cols, float fx, float fy, float cx,
                       float cy, float alpha_min) {
  GS_REQUIRE_DEV_IN(fn, depth); GS_REQUIRE_DEV_IN(fn, T);
  GS_REQUIRE_IN(fn, rows > 0 && cols > 0, "image size must be positive");
  GS_REQUIRE_IN(fn, alpha_min > 0.0f && alpha_min <= 1.0f, "alpha_min must lie in (0, 1]");
  GS_REQUIRE_IN(fn, std::isfinite(fx) && std::isfinite(fy) && std::isfinite(cx) && std::isfinite(cy),
                "the intrinsics must be finite");
  GS_REQUIRE_IN(fn, fx != 0.0f && fy != 0.0f, "fx and fy must not be 0");
  return GSPLAT_OK;
}

// The two losses do more per pixel than the depth regularisers (three-vectors, a square root or four exponentials, all
// in double): at gs::kRegBlocks blocks, one per CU, they wait on their own arithmetic, so they take up to eight times as
// many and the scratch of the partial sums is sized for that.
constexpr int kLossBlocks = 8 * gs::kRegBlocks;
int loss_blocks(long long n) { return (int)std::min<long long>(kLossBlocks, (n + 255) / 256); }

// the blocks' partial sums of a loss that was asked for its value (null otherwise)
int loss_partials(float *loss_out, double **partial) {
  *partial = nullptr;
  if (!loss_out) return GSPLAT_OK;
  gs::DeviceBuffer &acc = gs::scratch(gs::SCR_DEPTH_LOSS);
  if (int rc = acc.reserve(kLossBlocks * sizeof(double))) return rc;
  *partial = acc.as<double>();
  return GSPLAT_OK;
}

}  // namespace

extern "C" {

int gsplat_depth_to_normal(const float *depth, const float *T, int rows, int cols, float fx, float fy, float cx, float cy,
                           int inverse, float alpha_min, float *normal, void *stream) {
  if (int rc = check_stencil_args(__func__, depth, T, rows, cols, fx, fy, cx, cy, alpha_min)) return rc;
  GS_REQUIRE_DEV(normal);
  const Intrinsics k = {(double)fx, (double)fy, (double)cx, (double)cy};
  const dim3 grid(gs::div_up(cols, kNW), gs::div_up(rows, kNH)), block(kNW, kNRows);
  depth_to_normal_kernel<<<grid, block, 0, (hipStream_t)stream>>>(depth, T, rows, cols, k, inverse != 0, (double)alpha_min,
                                                                  normal);
  GS_LAUNCH_CHECK();
  return GSPLAT_OK;
}

int gsplat_depth_to_normal_backward(const float *depth, const float *T, int rows, int cols, float fx, float fy, float cx,
                                    float cy, int inverse, float alpha_min, const float *grad_normal, int accumulate,
                                    float *grad_depth, float *grad_alpha, void *stream) {
  if (int rc = check_stencil_args(__func__, depth, T, rows, cols, fx, fy, cx, cy, alpha_min)) return rc;
  GS_REQUIRE_DEV(grad_normal);
  if (grad_depth) GS_REQUIRE_DEV(grad_depth);
  if (grad_alpha) GS_REQUIRE_DEV(grad_alpha);
  if (!grad_depth && !grad_alpha) return GSPLAT_OK;
  const Intrinsics k = {(double)fx, (double)fy, (double)cx, (double)cy};
  const dim3 grid(gs::div_up(cols, kNW), gs::div_up(rows, kNH)), block(kNW, kNRows);
  hipStream_t st = (hipStream_t)stream;
  if (accumulate)
    depth_to_normal_backward_kernel<true><<<grid, block, 0, st>>>(depth, T, rows, cols, k, inverse != 0, (double)alpha_min,
                                                                  grad_normal, grad_depth, grad_alpha);
  else
    depth_to_normal_backward_kernel<false><<<grid, block, 0, st>>>(depth, T, rows, cols, k, inverse != 0, (double)alpha_min,
                                                                   grad_normal, grad_depth, grad_alpha);
  GS_LAUNCH_CHECK();
  return GSPLAT_OK;
}

int gsplat_normal_prior_loss(const float *normal, const float *prior, int rows, int cols, float weight, int accumulate,
                             float *grad_normal, float *loss_out, void *stream) {
  GS_REQUIRE_DEV(normal); GS_REQUIRE_DEV(prior);
  if (grad_normal) GS_REQUIRE_DEV(grad_normal);
  if (loss_out) GS_REQUIRE_DEV(loss_out);
  GS_REQUIRE(rows > 0 && cols > 0, "image size must be positive");
  hipStream_t st = (hipStream_t)stream;
  const long long n = (long long)rows * cols;
  const double scale = (double)weight / (double)n;
  const int blocks = loss_blocks(n);
  gs::ScratchLock lock;
  double *partial;
  if (int rc = loss_partials(loss_out, &partial)) return rc;
  if (accumulate) normal_prior_loss_kernel<true><<<blocks, 256, 0, st>>>(n, normal, prior, scale, grad_normal, partial);
  else normal_prior_loss_kernel<false><<<blocks, 256, 0, st>>>(n, normal, prior, scale, grad_normal, partial);
  GS_LAUNCH_CHECK();
  if (loss_out) {
    gs::reg_loss_finish_kernel<<<1, 64, 0, st>>>(partial, blocks, scale, loss_out);
    GS_LAUNCH_CHECK();
  }
  return GSPLAT_OK;
}

int gsplat_normal_smoothness_loss(const float *normal, const float *image, int rows, int cols, float weight,
                                  float edge_scale, int accumulate, float *grad_normal, float *loss_out, void *stream) {
  GS_REQUIRE_DEV(normal);
  if (image) GS_REQUIRE_DEV(image);
  if (grad_normal) GS_REQUIRE_DEV(grad_normal);
  if (loss_out) GS_REQUIRE_DEV(loss_out);
  GS_REQUIRE(rows > 0 && cols > 0, "image size must be positive");
  GS_REQUIRE(std::isfinite(edge_scale), "edge_scale must be finite");
  hipStream_t st = (hipStream_t)stream;
  const long long n = (long long)rows * cols;
  const double scale = (double)weight / (double)n;
  const int blocks = loss_blocks(n);
  gs::ScratchLock lock;
  double *partial;
  if (int rc = loss_partials(loss_out, &partial)) return rc;
  if (accumulate)
    normal_smoothness_loss_kernel<true><<<blocks, 256, 0, st>>>(rows, cols, normal, image, (double)edge_scale, scale,
                                                                grad_normal, partial);
  else
    normal_smoothness_loss_kernel<false><<<blocks, 256, 0, st>>>(rows, cols, normal, image, (double)edge_scale, scale,
                                                                 grad_normal, partial);
  GS_LAUNCH_CHECK();
  if (loss_out) {
    gs::reg_loss_finish_kernel<<<1, 64, 0, st>>>(partial, blocks, scale, loss_out);
    GS_LAUNCH_CHECK();
  }
  return GSPLAT_OK;
}

}  // extern "C"
