// gs_exchange.hip -- the multi-GPU gradient exchange's device side (3dgs_amd/dist.py): the kernels that pack a view's
// gradients into the rows the ranks sum (global, factored and split layouts), unpack the sums, and scatter or copy the
// compositing backward's rows to global order; and the entry points that are nothing but one of those launches.
#include "gs_context.h"
#include "gs_launch.h"
#include "gs_math.h"
#include "gs_rows.h"

namespace {

constexpr int kBlock = 256;

// ---- global-order gradient rows for the view-sharded all-reduce
__global__ __launch_bounds__(kBlock) void pack_global_kernel(const unsigned char *__restrict__ mask,
                                                             const int *__restrict__ rank, int N, int n_coeffs,
                                                             gsplat_gradients gr, float *__restrict__ packed) {
  const int width = 12 + 3 * n_coeffs;
  const long long e = (long long)blockIdx.x * kBlock + threadIdx.x;
  if (e >= (long long)N * width) return;
  const int i = (int)(e / width), k = (int)(e % width);
  float val = 0.0f;
  if (mask[i]) {
    const size_t j = (size_t)rank[i];
    const int n_rest3 = 3 * (n_coeffs - 1);
    if (k < 3) val = gr.grad_xyz[3 * j + k];
    else if (k < 6) val = gr.grad_rgb[3 * j + (k - 3)];
    else if (k < 6 + n_rest3) val = gr.grad_sh[j * n_rest3 + (k - 6)];
    else if (k == 6 + n_rest3) val = gr.grad_opacity[j];
    else if (k < 10 + n_rest3) val = gr.grad_scale[3 * j + (k - 7 - n_rest3)];
    else if (k < 14 + n_rest3) val = gr.grad_quaternion[4 * j + (k - 10 - n_rest3)];
    else val = 1.0f;
  }
  packed[e] = val;
}

// ---- factored exchange rows (view-sharded training).  Every SH-coefficient gradient of a view is the outer product
// g_rgb (3) x Y_k(view direction): instead of shipping 3*n_coeffs floats per gaussian through the all-reduce, a
// rank ships only its g_rgb in a slot of its own (3 floats; the other ranks' slots stay zero, so the SUM all-reduce
// acts as an all-gather for those columns) and every rank rebuilds sum_r g_rgb^r * Y_k(dir^r) locally from the
// camera positions.  Row layout: [xyz3 | opacity1 | scale3 | quat4 | visible1 | g_rgb slot 0 .. slot W-1].
__global__ __launch_bounds__(kBlock) void pack_factored_kernel(const unsigned char *__restrict__ mask,
                                                               const int *__restrict__ rank_of, int N, int my_rank,
                                                               int world, gsplat_gradients gr,
                                                               float *__restrict__ packed) {
  const int width = 12 + 3 * world;
  const long long e = (long long)blockIdx.x * kBlock + threadIdx.x;
  if (e >= (long long)N * width) return;
  const int i = (int)(e / width), k = (int)(e % width);
  float val = 0.0f;
  if (mask[i]) {
    const size_t j = (size_t)rank_of[i];
    if (k < 3) val = gr.grad_xyz[3 * j + k];
    else if (k == 3) val = gr.grad_opacity[j];
    else if (k < 7) val = gr.grad_scale[3 * j + (k - 4)];
    else if (k < 11) val = gr.grad_quaternion[4 * j + (k - 7)];
    else if (k == 11) val = 1.0f;
    else if ((k - 12) / 3 == my_rank) val = gr.grad_precompute_rgb[3 * j + (k - 12) % 3];
  }
  packed[e] = val;
}

template <int L>
__global__ __launch_bounds__(kBlock) void unpack_factored_kernel(const float *__restrict__ xyz,
                                                                 const float *__restrict__ campos_all, int N,
                                                                 int world, const float *__restrict__ packed,
                                                                 float *__restrict__ full) {
  constexpr int n = (L + 1) * (L + 1);
  const int i = blockIdx.x * kBlock + threadIdx.x;
  if (i >= N) return;
  const int wf = 12 + 3 * world, wo = 12 + 3 * n;
  const float *row = packed + (size_t)i * wf;
  float *out = full + (size_t)i * wo;
  float acc[n][3];
#pragma unroll
  for (int k = 0; k < n; ++k) acc[k][0] = acc[k][1] = acc[k][2] = 0.0f;
  const float px = xyz[3 * i], py = xyz[3 * i + 1], pz = xyz[3 * i + 2];
  for (int r = 0; r < world; ++r) {
    const float g0 = row[12 + 3 * r], g1 = row[13 + 3 * r], g2 = row[14 + 3 * r];
    if (g0 == 0.0f && g1 == 0.0f && g2 == 0.0f) continue;
    float dx, dy, dz, len, Y[n];
    gs::view_dir(px, py, pz, campos_all[3 * r], campos_all[3 * r + 1], campos_all[3 * r + 2], dx, dy, dz, len);
    gs::sh_basis<L>(dx, dy, dz, Y);
#pragma unroll
    for (int k = 0; k < n; ++k) { acc[k][0] += g0 * Y[k]; acc[k][1] += g1 * Y[k]; acc[k][2] += g2 * Y[k]; }
  }
  out[0] = row[0]; out[1] = row[1]; out[2] = row[2];  // xyz
#pragma unroll
  for (int k = 0; k < n; ++k) { out[3 + 3 * k] = acc[k][0]; out[4 + 3 * k] = acc[k][1]; out[5 + 3 * k] = acc[k][2]; }
  out[3 + 3 * n] = row[3];                                             // opacity
  out[4 + 3 * n] = row[4]; out[5 + 3 * n] = row[5]; out[6 + 3 * n] = row[6];  // scale
  out[7 + 3 * n] = row[7]; out[8 + 3 * n] = row[8]; out[9 + 3 * n] = row[9]; out[10 + 3 * n] = row[10];  // quaternion
  out[11 + 3 * n] = row[11];                                           // visibility count
}

// g_rgb of this view in global gaussian order, straight from the compositing backward's rows (rows[j][0..2]):
// available before the per-gaussian backward has run, so its all-gather can overlap that kernel.
__global__ __launch_bounds__(kBlock) void scatter_rgb_rows_kernel(const unsigned char *__restrict__ mask,
                                                                  const int *__restrict__ rank_of, int N,
                                                                  const float *__restrict__ rows,
                                                                  float *__restrict__ rgb, float *__restrict__ common,
                                                                  float *__restrict__ uv_norm) {
  const long long e = (long long)blockIdx.x * kBlock + threadIdx.x;
  if (e >= (long long)N * 3) return;
  const int i = (int)(e / 3), k = (int)(e % 3);
  const bool kept = mask[i] != 0;
  rgb[e] = kept ? rows[(size_t)rank_of[i] * 16 + k] : 0.0f;
  // r05: the exchange's twelve common columns are written in place by preprocess_bwd_kernel for the gaussians this view
  // saw; the rows of the culled ones are cleared here (thread k of a row: its k-th 16 bytes), where the mask is read anyway
  if (common && !kept) {
    reinterpret_cast<gs::f4u *>(common + (size_t)i * 12)[k] = gs::f4u{0.0f, 0.0f, 0.0f, 0.0f};
    if (uv_norm && k == 0) uv_norm[i] = 0.0f;
  }
}

// |grad_uv| of this view in global gaussian order (0 where culled): the densification statistic of a view-sharded step
__global__ __launch_bounds__(kBlock) void pack_uv_norm_kernel(const unsigned char *__restrict__ mask,
                                                              const int *__restrict__ rank_of, int N,
                                                              const float *__restrict__ grad_uv,
                                                              float *__restrict__ out) {
  const int i = blockIdx.x * kBlock + threadIdx.x;
  if (i >= N) return;
  float val = 0.0f;
  if (mask[i]) {
    const float2 g = reinterpret_cast<const float2 *>(grad_uv)[rank_of[i]];
    val = sqrtf(g.x * g.x + g.y * g.y);
  }
  out[i] = val;
}

// absgrad mode: the norm of row slots 10 and 11 (the absolute sums of the pixels' shares of dL/d uv) in global gaussian
// order, 0 where culled -- pack_uv_norm_kernel's counterpart, in preprocess_bwd_kernel<.., kAbsRow>'s expression
__global__ __launch_bounds__(kBlock) void pack_abs_norm_kernel(const unsigned char *__restrict__ mask,
                                                               const int *__restrict__ rank_of, int N,
                                                               const float4 *__restrict__ rows, float *__restrict__ out) {
  const int i = blockIdx.x * kBlock + threadIdx.x;
  if (i >= N) return;
  float val = 0.0f;
  if (mask[i]) {
    const float4 c = rows[4 * (size_t)rank_of[i] + 2];
    val = sqrtf(c.z * c.z + c.w * c.w);
  }
  out[i] = val;
}

// ... and the two sums themselves, compacted order
__global__ __launch_bounds__(kBlock) void copy_abs_uv_kernel(const float4 *__restrict__ rows, int M, float2 *__restrict__ out) {
  const int j = blockIdx.x * kBlock + threadIdx.x;
  if (j >= M) return;
  const float4 c = rows[4 * (size_t)j + 2];
  out[j] = make_float2(c.z, c.w);
}

// Split exchange: the 12 direction-independent columns (SUM all-reduce) and this view's g_rgb (all-gather).
__global__ __launch_bounds__(kBlock) void pack_split_kernel(const unsigned char *__restrict__ mask,
                                                            const int *__restrict__ rank_of, int i_first, int N,
                                                            gsplat_gradients gr, float *__restrict__ common,
                                                            float *__restrict__ rgb) {
  const int i = i_first + blockIdx.x * kBlock + threadIdx.x;  // one gaussian per thread: three 16-byte stores per row
  if (i >= N) return;
  gs::f4u r0 = {0.0f, 0.0f, 0.0f, 0.0f}, r1 = r0, r2 = r0;
  float c0 = 0.0f, c1 = 0.0f, c2 = 0.0f;
  if (mask[i]) {
    const size_t j = (size_t)rank_of[i];
    const float *gq = gr.grad_quaternion + 4 * j;
    r0 = gs::f4u{gr.grad_xyz[3 * j], gr.grad_xyz[3 * j + 1], gr.grad_xyz[3 * j + 2], gr.grad_opacity[j]};
    r1 = gs::f4u{gr.grad_scale[3 * j], gr.grad_scale[3 * j + 1], gr.grad_scale[3 * j + 2], gq[0]};
    r2 = gs::f4u{gq[1], gq[2], gq[3], 1.0f};
    if (rgb) {
      c0 = gr.grad_precompute_rgb[3 * j]; c1 = gr.grad_precompute_rgb[3 * j + 1]; c2 = gr.grad_precompute_rgb[3 * j + 2];
    }
  }
  gs::f4u *row = reinterpret_cast<gs::f4u *>(common + (size_t)i * 12);
  row[0] = r0; row[1] = r1; row[2] = r2;
  if (rgb) { rgb[(size_t)i * 3] = c0; rgb[(size_t)i * 3 + 1] = c1; rgb[(size_t)i * 3 + 2] = c2; }
}

// rgb_all: world blocks of `stride` floats; block r = [N,3] g_rgb of rank r followed by that rank's campos[3].
// kSh: rebuild the SH-coefficient columns from rgb_all; kCommon: place the twelve all-reduced columns.  The two
// halves touch disjoint columns of `full`, so the SH half can run while the all-reduce of `common` is in flight.
template <int L, bool kSh, bool kCommon>
__global__ __launch_bounds__(kBlock) void unpack_split_kernel(const float *__restrict__ xyz, int N, int world,
                                                              const float *__restrict__ common,
                                                              const float *__restrict__ rgb_all, size_t stride,
                                                              float *__restrict__ full) {
  constexpr int n = (L + 1) * (L + 1);
  constexpr int wo = 12 + 3 * n;
  const int i = blockIdx.x * kBlock + threadIdx.x;
  if constexpr (!kSh) {  // the twelve all-reduced columns only: two short pieces per row
    if (i >= N) return;
    float *out = full + (size_t)i * wo;
    const float *row = common + (size_t)i * 12;
    out[0] = row[0]; out[1] = row[1]; out[2] = row[2];                          // xyz
    out[3 + 3 * n] = row[3];                                                    // opacity
    out[4 + 3 * n] = row[4]; out[5 + 3 * n] = row[5]; out[6 + 3 * n] = row[6];  // scale
    out[7 + 3 * n] = row[7]; out[8 + 3 * n] = row[8]; out[9 + 3 * n] = row[9]; out[10 + 3 * n] = row[10];  // quaternion
    out[11 + 3 * n] = row[11];                                                  // visibility count
  } else {
    // The rebuilt rows leave through LDS, one row per wave instruction (a lane storing ITS 240-byte row touches 64
    // cache lines per instruction).  kCols floats of every row are written, starting at column kFirst.
    constexpr int kCols = kCommon ? wo : 3 * n, kFirst = kCommon ? 0 : 3, kPitch = kCols | 1;  // odd pitch: no bank conflicts
    __shared__ float s_rows[kBlock * kPitch];
    const int lane = threadIdx.x & 63, wave_first = threadIdx.x - lane;
    const int iw = blockIdx.x * kBlock + wave_first;
    if (iw >= N) return;
    float *mine = s_rows + (wave_first + lane) * kPitch;
    if (i < N) {
      float acc[n][3];
#pragma unroll
      for (int k = 0; k < n; ++k) acc[k][0] = acc[k][1] = acc[k][2] = 0.0f;
      const float px = xyz[3 * i], py = xyz[3 * i + 1], pz = xyz[3 * i + 2];
      for (int r = 0; r < world; ++r) {
        const float *blk = rgb_all + (size_t)r * stride;
        const float g0 = blk[3 * (size_t)i], g1 = blk[3 * (size_t)i + 1], g2 = blk[3 * (size_t)i + 2];
        if (g0 == 0.0f && g1 == 0.0f && g2 == 0.0f) continue;
        const float *cp = blk + 3 * (size_t)N;
        float dx, dy, dz, len, Y[n];
        gs::view_dir(px, py, pz, cp[0], cp[1], cp[2], dx, dy, dz, len);
        gs::sh_basis<L>(dx, dy, dz, Y);
#pragma unroll
        for (int k = 0; k < n; ++k) { acc[k][0] += g0 * Y[k]; acc[k][1] += g1 * Y[k]; acc[k][2] += g2 * Y[k]; }
      }
      constexpr int o = 3 - kFirst;  // where the SH block starts inside the staged row
#pragma unroll
      for (int k = 0; k < n; ++k) { mine[o + 3 * k] = acc[k][0]; mine[o + 3 * k + 1] = acc[k][1]; mine[o + 3 * k + 2] = acc[k][2]; }
      if constexpr (kCommon) {
        const float *row = common + (size_t)i * 12;
        mine[0] = row[0]; mine[1] = row[1]; mine[2] = row[2];
#pragma unroll
        for (int k = 3; k < 12; ++k) mine[3 * n + k] = row[k];
      }
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
    const int rows = min(64, N - iw);
    const float *wrows = s_rows + wave_first * kPitch;
    float *dst = full + (size_t)iw * wo + kFirst;
    if constexpr (kCols <= 64) {
      for (int r = 0; r < rows; ++r)
        if (lane < kCols) dst[(size_t)r * wo + lane] = wrows[r * kPitch + lane];
    } else {
      static_assert(kCols <= 128, "row wider than two wave instructions");
      for (int r = 0; r < rows; ++r) {
        dst[(size_t)r * wo + lane] = wrows[r * kPitch + lane];
        if (lane + 64 < kCols) dst[(size_t)r * wo + lane + 64] = wrows[r * kPitch + lane + 64];
      }
    }
  }
}

}  // namespace

namespace gs {

int launch_scatter_rgb_rows(const unsigned char *mask, const int *rank, int N, const float *rows, float *rgb_global,
                            float *common, float *uv_norm, hipStream_t st) {
  scatter_rgb_rows_kernel<<<div_up((long long)N * 3, kBlock), kBlock, 0, st>>>(mask, rank, N, rows, rgb_global, common, uv_norm);
  GS_LAUNCH_CHECK();
  return GSPLAT_OK;
}

}  // namespace gs

extern "C" {

int gsplat_packed_gradient_width(int l_max) { return 12 + 3 * (l_max + 1) * (l_max + 1); }
int gsplat_factored_gradient_width(int world_size) { return 12 + 3 * world_size; }

int gsplat_pack_gradients_factored(gsplat_context *c, const gsplat_gradients *grads, int num_gaussians, int rank,
                                   int world_size, float *packed, void *stream) {
  GS_REQUIRE(c && grads, "null argument struct");
  GS_REQUIRE(c->have_forward && num_gaussians == c->N, "does not match the recorded forward");
  GS_REQUIRE(world_size >= 1 && rank >= 0 && rank < world_size, "bad rank / world_size");
  GS_REQUIRE_DEV(packed);
  GS_REQUIRE_DEV(grads->grad_precompute_rgb);  // backward must have been asked for this intermediate
  const long long total = (long long)num_gaussians * (12 + 3 * world_size);
  pack_factored_kernel<<<gs::div_up(total, kBlock), kBlock, 0, (hipStream_t)stream>>>(
      c->mask.as<unsigned char>(), c->rank.as<int>(), num_gaussians, rank, world_size, *grads, packed);
  GS_LAUNCH_CHECK();
  return GSPLAT_OK;
}

int gsplat_unpack_gradients_factored(const float *xyz, const float *campos_all, const float *packed, int l_max,
                                     int num_gaussians, int world_size, float *full, void *stream) {
  GS_REQUIRE_DEV(xyz); GS_REQUIRE_DEV(campos_all); GS_REQUIRE_DEV(packed); GS_REQUIRE_DEV(full);
  GS_REQUIRE(l_max >= 0 && l_max <= 3 && num_gaussians >= 0 && world_size >= 1, "bad sizes");
  if (num_gaussians == 0) return GSPLAT_OK;
  const dim3 g(gs::div_up(num_gaussians, kBlock)), b(kBlock);
  hipStream_t st = (hipStream_t)stream;
  gs::with_degree<0>(l_max, [&](auto L) {
    unpack_factored_kernel<decltype(L)::value><<<g, b, 0, st>>>(xyz, campos_all, num_gaussians, world_size, packed, full);
  });
  GS_LAUNCH_CHECK();
  return GSPLAT_OK;
}

int gsplat_pack_gradients_split_range(gsplat_context *c, const gsplat_gradients *grads, int num_gaussians,
                                      int first_gaussian, int end_gaussian, float *common, float *rgb, void *stream) {
  GS_REQUIRE(c && grads, "null argument struct");
  GS_REQUIRE(c->have_forward && num_gaussians == c->N, "does not match the recorded forward");
  GS_REQUIRE(0 <= first_gaussian && first_gaussian <= end_gaussian && end_gaussian <= num_gaussians, "bad gaussian range");
  GS_REQUIRE_DEV(common);
  if (rgb) {
    GS_REQUIRE_DEV(rgb);
    GS_REQUIRE_DEV(grads->grad_precompute_rgb);  // backward must have been asked for this intermediate
  }
  if (end_gaussian == first_gaussian) return GSPLAT_OK;
  pack_split_kernel<<<gs::div_up((long long)(end_gaussian - first_gaussian), kBlock), kBlock, 0, (hipStream_t)stream>>>(
      c->mask.as<unsigned char>(), c->rank.as<int>(), first_gaussian, end_gaussian, *grads, common, rgb);
  GS_LAUNCH_CHECK();
  return GSPLAT_OK;
}

int gsplat_pack_gradients_split(gsplat_context *c, const gsplat_gradients *grads, int num_gaussians, float *common,
                                float *rgb, void *stream) {
  return gsplat_pack_gradients_split_range(c, grads, num_gaussians, 0, num_gaussians, common, rgb, stream);
}

int gsplat_pack_uv_grad_norm(gsplat_context *c, const gsplat_gradients *grads, int num_gaussians, float *uv_norm,
                             void *stream) {
  GS_REQUIRE(c && grads, "null argument struct");
  GS_REQUIRE(c->have_forward && num_gaussians == c->N, "does not match the recorded forward");
  GS_REQUIRE_DEV(uv_norm);
  GS_REQUIRE_DEV(grads->grad_uv);  // backward must have been asked for this intermediate
  pack_uv_norm_kernel<<<gs::div_up((long long)num_gaussians, kBlock), kBlock, 0, (hipStream_t)stream>>>(
      c->mask.as<unsigned char>(), c->rank.as<int>(), num_gaussians, grads->grad_uv, uv_norm);
  GS_LAUNCH_CHECK();
  return GSPLAT_OK;
}

int gsplat_unpack_gradients_split(const float *xyz, const float *common, const float *rgb_all, size_t rank_stride,
                                  int l_max, int num_gaussians, int world_size, float *full, void *stream) {
  GS_REQUIRE_DEV(full);
  GS_REQUIRE(common != nullptr || rgb_all != nullptr, "nothing to unpack");
  GS_REQUIRE(l_max >= 0 && l_max <= 3 && num_gaussians >= 0 && world_size >= 1, "bad sizes");
  if (common) GS_REQUIRE_DEV(common);
  if (rgb_all) {
    GS_REQUIRE_DEV(rgb_all); GS_REQUIRE_DEV(xyz);
    GS_REQUIRE(rank_stride >= 3 * (size_t)num_gaussians + 3, "rank_stride must cover [N,3] g_rgb + campos[3]");
  }
  if (num_gaussians == 0) return GSPLAT_OK;
  const dim3 g(gs::div_up(num_gaussians, kBlock)), b(kBlock);
  hipStream_t st = (hipStream_t)stream;
  gs::with_degree<0>(l_max, [&](auto L) {
    auto launch = [&](auto kernel, const float *xyz_in, const float *common_in, const float *rgb_in, size_t stride) {
      kernel<<<g, b, 0, st>>>(xyz_in, num_gaussians, world_size, common_in, rgb_in, stride, full);
    };
    constexpr int kL = decltype(L)::value;
    if (common && rgb_all) launch(unpack_split_kernel<kL, true, true>, xyz, common, rgb_all, rank_stride);
    else if (rgb_all) launch(unpack_split_kernel<kL, true, false>, xyz, nullptr, rgb_all, rank_stride);
    else launch(unpack_split_kernel<kL, false, true>, nullptr, common, nullptr, 0);
  });
  GS_LAUNCH_CHECK();
  return GSPLAT_OK;
}

int gsplat_pack_gradients_global(gsplat_context *c, const gsplat_gradients *grads, int l_max, int num_gaussians,
                                 float *packed, void *stream) {
  GS_REQUIRE(c && grads, "null argument struct");
  GS_REQUIRE(c->have_forward && num_gaussians == c->N && l_max == c->l_max, "does not match the recorded forward");
  GS_REQUIRE_DEV(packed);
  const int n_coeffs = (l_max + 1) * (l_max + 1);
  const long long total = (long long)num_gaussians * (12 + 3 * n_coeffs);
  pack_global_kernel<<<gs::div_up(total, kBlock), kBlock, 0, (hipStream_t)stream>>>(
      c->mask.as<unsigned char>(), c->rank.as<int>(), num_gaussians, n_coeffs, *grads, packed);
  GS_LAUNCH_CHECK();
  return GSPLAT_OK;
}

int gsplat_context_absgrad_uv(gsplat_context *c, float *abs_uv, void *stream) {
  GS_REQUIRE(c != nullptr, "null context");
  GS_REQUIRE(!c->render_only, "a render-only context has no backward");
  GS_REQUIRE(c->have_forward && c->rows_ready, "no compositing backward since the last forward");
  GS_REQUIRE(c->rows_abs, "the last compositing backward did not run in absgrad mode (gsplat_context_set_absgrad)");
  if (c->M == 0) return GSPLAT_OK;
  GS_REQUIRE_DEV(abs_uv);
  GS_REQUIRE(((uintptr_t)abs_uv & 7) == 0, "abs_uv must be 8-byte aligned");
  copy_abs_uv_kernel<<<gs::div_up((long long)c->M, kBlock), kBlock, 0, (hipStream_t)stream>>>(
      c->grad_rows.as<float4>(), c->M, reinterpret_cast<float2 *>(abs_uv));
  GS_LAUNCH_CHECK();
  return GSPLAT_OK;
}

int gsplat_pack_absgrad_norm(gsplat_context *c, int num_gaussians, float *uv_norm, void *stream) {
  GS_REQUIRE(c != nullptr, "null context");
  GS_REQUIRE(!c->render_only, "a render-only context has no backward");
  GS_REQUIRE(c->have_forward && c->rows_ready, "no compositing backward since the last forward");
  GS_REQUIRE(c->rows_abs, "the last compositing backward did not run in absgrad mode (gsplat_context_set_absgrad)");
  GS_REQUIRE(num_gaussians == c->N, "does not match the recorded forward");
  GS_REQUIRE_DEV(uv_norm);
  pack_abs_norm_kernel<<<gs::div_up((long long)num_gaussians, kBlock), kBlock, 0, (hipStream_t)stream>>>(
      c->mask.as<unsigned char>(), c->rank.as<int>(), num_gaussians, c->grad_rows.as<float4>(), uv_norm);
  GS_LAUNCH_CHECK();
  return GSPLAT_OK;
}

}  // extern "C"
