// gs_preprocess_bwd.hip -- the per-gaussian backward of the device-resident pass (gsplat_backward_gaussians*, gs_fused.hip):
// one fused kernel for the whole SH / conic / Jacobian / Sigma / projection chain, optionally with the Adam step inside,
// the second half of the camera gradient, and the SH group's Adam step in a kernel of its own.  Kernels first, their
// launchers (gs_launch.h; arguments: gs_pergaussian_args.h) at the end.  Nothing here knows the context.
#include "gs_common.h"
#include "gs_launch.h"
#include "gs_math.h"
#include "gs_pergaussian_args.h"
#include "gs_render.h"
#include "gs_rows.h"

namespace {

constexpr int kBlock = 256;

struct BwdOut {
  float *xyz, *rgb, *sh, *opacity, *scale, *quaternion;
  float *conic, *uv, *J, *sigma, *xyz_c, *pre_rgb;
  // r05, view-sharded step: instead of the six compacted leaf arrays the kernel writes the row the exchange sums --
  // common[i] = {xyz 3, opacity, scale 3, quaternion 4, 1.0 (this view saw the gaussian)} at the gaussian's GLOBAL index i
  // (48 bytes, three 16-byte stores) -- and |grad_uv| at uv_norm[i]; the rows of culled gaussians were zeroed by
  // gsplat_backward_render_split.  No compacted gradient array, no pack pass.
  float *common, *uv_norm;
};

// Number of entries of the increasing array c2g[0..M) that are below `key` = the first compacted slot whose global index
// is >= key.  A 64-ary search by the whole wave: every step the lanes probe 64 evenly spaced entries and a ballot keeps
// the one sub-interval that contains the answer (four steps of one load each at 1e6 gaussians; every wave of the
// grid does it for itself, no barrier).
__device__ __forceinline__ int first_slot_not_below(const int *__restrict__ c2g, int M, int key) {
  const int lane = threadIdx.x & 63;
  int lo = 0, hi = M;  // c2g[j] < key for j < lo, c2g[j] >= key for j >= hi
  while (hi > lo) {
    const int step = (hi - lo + 63) >> 6;
    const long long p = (long long)lo + (long long)lane * step;
    const bool below = p < hi && c2g[p] < key;
    const int t = __popcll(__ballot(below));  // the array is increasing: the first t probes are below the key
    if (t == 0) {
      hi = lo;
    } else {
      const long long next = (long long)lo + (long long)t * step;  // the probe after the last one below (if it exists)
      hi = next < hi ? (int)next : hi;
      lo = lo + (t - 1) * step + 1;
    }
  }
  return lo;
}

// r06: what the per-gaussian backward needs to apply the optimizer step itself (kAdam; gsplat_backward_gaussians_adam):
// the moments of the six parameter groups in GLOBAL order next to the parameters (`g`, updated in place), the groups'
// learning rates, Adam's constants and the densification statistics.
struct AdamFused {
  float *m_xyz, *v_xyz, *m_rgb, *v_rgb, *m_sh, *v_sh, *m_op, *v_op, *m_sc, *v_sc, *m_q, *v_q;
  float lr_xyz, lr_rgb, lr_sh, lr_op, lr_sc, lr_q;
  float b1, b2, eps, bias1, bias2;
  float *uv_accum;
  int *accum_dur;
  float *dir;  // kAdam 3: [M,3] d loss / d position through the view direction of the colour (sh_adam_dir_kernel -> here)
};

// ---- backward of everything per gaussian, one thread per compacted slot
// kAdam (r06, single-GPU training): the kernel applies the masked Adam step of TrainerImpl::optimizer_step
// (cuda/trainer.cu:1027-1158) to the gaussian it has just differentiated instead of storing six gradient arrays for a
// second and third kernel to read back next to parameters this one has just read.  A gaussian's gradients depend on its
// own parameters only, so updating in place is safe once the thread -- for the SH rows: the wave -- has read what it
// needs.  Gradient values and update are the separate kernels' (gs::sh_bwd's product, gs::adam_values): parameters and
// moments come out bit-identical to gsplat_backward_gaussians + gsplat_optimizer_step_sh_factored + gsplat_optimizer_step
// (tests/test_optimizer_gpu.py).  The SH group: the coefficient rows stay in the wave's LDS rows (gs::sh_bwd<L, false>),
// every lane parks its direction and colour gradient next to them, and the wave walks its 64 rows element by element --
// thread e owns element e of the span, rebuilds gradient = g_rgb[channel] * Y_k(direction) as
// optimizer_sh_factored_kernel does and streams sh / exp_avg / exp_avg_sq through the update: consecutive lanes,
// consecutive addresses.
// kAdam 2: all six groups here.  kAdam 1: band 0, opacity, scale, rotation and the statistics here; the SH group
// (gsplat_optimizer_step_sh_factored, which needs the positions the backward saw) and the position group
// (gsplat_optimizer_step on grad_xyz) stay with the optimizer kernels behind this one.  kAdam 3: the five small groups
// here and NOTHING of the SH rows -- sh_adam_dir_kernel (below) has run in front of this kernel: it read the coefficient
// rows once, for their Adam step AND for sh_bwd's sums over them, and left the position gradient through the view
// direction in ad.dir; no LDS, and without sh_bwd's basis tables far fewer registers.
#ifndef GS_BWD3_WAVES
#define GS_BWD3_WAVES 3  // waves per SIMD the kAdam 3 form is compiled for (r06 A/B)
#endif
// kDepthRow: the rows carry dL/dz of the composited depth in slot 9 (gsplat_backward_render_depth; gs_render.h:
// DepthMaps) -- a template flag, so that the default instantiations stay exactly what they were
// kCamGrad (plain form only, whole range): every wave also sums its gaussians' shares of dL/d view[0..11] and
// dL/d campos in double and one lane stores them as row (first slot / 64) of cam_rows [ceil(M/64), 16];
// cam_grad_finalize_kernel sums the rows (gsplat_backward_gaussians_camera)
// kAbsRow: the rows carry the absolute sums of the pixels' shares of dL/d uv in slots 10 and 11 (absgrad mode,
// gsplat_context_set_absgrad), and the densification statistic -- uv_norm of the split form, uv_grad_accum of the Adam
// forms -- is their norm instead of |grad_uv|; every gradient is what it is without the flag.  (The camera form stores no
// statistic and has no such instantiation.)
// kAntialias (plain form only; gsplat_context_set_antialiased): the recorded forward's records carried o = sigmoid(logit) *
// rho, so row slot 3 is g_eff = dL/d logit(o).  rho is recomputed with the forward's function on the forward's inputs (bit
// for bit its value, like Sigma, J and the conic); g_eff becomes dL/d logit and dL/d rho (gs::effective_opacity_bwd), and
// dL/d rho enters conic_bwd as a covariance term (gs::compensation_bwd) -- dJ, dSigma and everything behind them take it
// through the code that is there.
// kDirSums (the plain form and kAdam 1; gsplat_context_set_dir_sums): the recorded forward left gs::sh_dir_sums of every kept gaussian
// in dir_sums [M,9] (preprocess_kernel<.., kDirSums>).  The coefficient rows, band 0 and xyz_c are then not read at all:
// the coefficient gradients g_rgb[c] * Y_k need no coefficient, the position gradient through the view direction is
// gs::sh_dir_finish of the nine loaded sums, and the camera-space position is gs::camera_space of the position this kernel
// loads anyway -- the forward's function on the forward's inputs, bit for bit what it stored.  204 bytes per gaussian
// become 36; every result is the bits of the form without the flag.  kAdam 1 (the trainer's default iteration) stores no
// coefficient gradients, so with the flag it touches neither the rows nor the LDS: its SH group is stepped by
// gsplat_optimizer_step_sh_factored behind it, which reads the rows for the update it makes.
template <int L, int kAdam = 0, bool kDepthRow = false, bool kCamGrad = false, bool kAbsRow = false, bool kAntialias = false,
          bool kDirSums = false>
__global__ __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(kAdam == 3 ? GS_BWD3_WAVES : 3, 8))) void preprocess_bwd_kernel(gsplat_gaussians g, const float *__restrict__ view,
                                                                const float *__restrict__ proj, int M,
                                                                const int *__restrict__ c2g,
                                                                const float *__restrict__ xyz_c_sel,
                                                                const float4 *__restrict__ rows_in, float fx, float fy,
                                                                float tan_fovx, float tan_fovy, float fwd_tan_fovx,
                                                                float fwd_tan_fovy, float mh_dist, float cx, float cy,
                                                                float cz, int width, int height, BwdOut o,
                                                                int ranged, int i_lo, int i_hi, AdamFused ad,
                                                                double *__restrict__ cam_rows,
                                                                const float *__restrict__ dir_sums) {
  static_assert(!kDirSums || ((kAdam == 0 || kAdam == 1) && !kCamGrad && !kAntialias),
                "the direction sums are read by the plain form and by kAdam 1 only");
  static_assert(!kCamGrad || kAdam == 0, "the camera gradient is a form of the plain backward");
  static_assert(!(kCamGrad && kAbsRow), "the camera form stores no densification statistic");
  static_assert(!kAntialias || (kAdam == 0 && !kCamGrad), "anti-aliased mode is a form of the plain backward");
  // ranged: only the gaussians with global index in [i_lo, i_hi), i.e. the compacted slots [first slot whose global index
  // is >= i_lo, first slot whose global index is >= i_hi) (chunked backward of a view-sharded step: the exchange of one
  // chunk runs while the next is computed); the grid covers the largest possible chunk, blocks past its end leave at once.
  // The two slots come from compact_to_global, which is increasing, NOT from rank[]: after a forward that walked the
  // compacted slots (preprocess_kernel<.., kCompact>) rank[i] of a CULLED index still holds the cull's slice-local
  // count, and a range bound may well be a culled index.
  int j_first = 0;
  if (ranged) {
    j_first = first_slot_not_below(c2g, M, i_lo);
    M = first_slot_not_below(c2g, M, i_hi);
  }
  const int j = j_first + blockIdx.x * kBlock + threadIdx.x;
  constexpr int n = (L + 1) * (L + 1), kRest = (n - 1) * 3;
  // The SH rows (kRest floats per gaussian, 180 B at degree 3) go through LDS: a lane reading ITS row touches 64
  // different cache lines per wave instruction; the wave's 64 rows as one linear span touch 8.  Same for the
  // gradient rows on the way out.  Each wave stages only its own rows (no workgroup barrier).
  __shared__ __attribute__((aligned(16))) float s_sh[kRest > 0 && kAdam != 3 && !(kDirSums && kAdam != 0) ? kBlock * kRest : 4];
  // kAdam: per row the unit direction and the colour gradient (what the SH gradients are made of) and the global row
  __shared__ float s_dir[kAdam == 2 && kRest > 0 ? kBlock * 7 : 1];
  const int lane = threadIdx.x & 63, wave_first = threadIdx.x - lane;
  const int jw = j_first + blockIdx.x * kBlock + wave_first;  // first compacted slot of this wave
  if (jw >= M) return;
  const int rows = min(64, M - jw);
  const bool live = j < M;
  const int i = c2g[live ? j : jw];
  float *wsh = s_sh + (kAdam != 3 && !(kDirSums && kAdam != 0) ? wave_first * kRest : 0);
  if constexpr (kRest > 0 && kAdam != 3 && !kDirSums) {
    const int i0 = __builtin_amdgcn_readfirstlane(i);
    if (__all(!live || i == i0 + lane)) {  // consecutive gaussians (no culling in between): one linear span
      gs::rows_to_lds<kRest>(g.sh + (size_t)i0 * kRest, wsh, rows, lane);
    } else {
      // Culled gaussians in between (every real training view): the wave's rows are scattered.  Twelve lanes fetch one
      // row -- eleven 16-byte pieces and the last float(s) -- so a wave instruction brings in five whole rows (880 B)
      // instead of one (180 B with one float per lane: 64 load instructions per wave, r01), and all of a wave's loads
      // are issued before the first LDS store.  Rows sit at a pitch of kRest words in LDS (conflict-free for the
      // per-lane walk of sh_bwd), which is not 16-byte aligned: the pieces are stored as four words.
      constexpr int kPieces = (kRest + 3) / 4, kPer = 64 / kPieces, kIter = (64 + kPer - 1) / kPer;
      static_assert(kPieces <= 64 && kPer >= 1, "row too long for one lane group");
      const int grp = lane / kPieces, piece = lane - grp * kPieces;
      const bool in_grp = grp < kPer;
      float4 v[kIter];
#pragma unroll
      for (int it = 0; it < kIter; ++it) {
        const int r = it * kPer + grp;
        const int ir = __shfl(i, r < rows ? r : 0, 64);
        v[it] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (in_grp && r < rows) {
          const float *src = g.sh + (size_t)ir * kRest + 4 * piece;
          if (4 * piece + 3 < kRest) {
            v[it] = __builtin_bit_cast(float4, *reinterpret_cast<const gs::f4u *>(src));
          } else {  // the row's last, partial piece
            v[it].x = src[0];
            if (4 * piece + 1 < kRest) v[it].y = src[1];
            if (4 * piece + 2 < kRest) v[it].z = src[2];
          }
        }
      }
#pragma unroll
      for (int it = 0; it < kIter; ++it) {
        const int r = it * kPer + grp;
        if (in_grp && r < rows) {
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
  }
  // (kAdam: the SH group first, while nothing else of the thread's state is live -- the kernel sits at the 168-register
  // step of three workgroups per CU; sh_bwd below still finds the coefficients in LDS, the update went to global memory)
  if constexpr (kRest > 0 && kAdam == 2) {
    {  // the direction exactly as gs::sh_bwd / optimizer_sh_factored_kernel form it (and the colour gradient: rows_in[.].xyz)
      const float4 ga = rows_in[4 * (live ? j : jw)];
      float ux, uy, uz, len;
      gs::view_dir(g.xyz[3 * i], g.xyz[3 * i + 1], g.xyz[3 * i + 2], cx, cy, cz, ux, uy, uz, len);
      float *d = s_dir + (wave_first + lane) * 7;
      d[0] = ux; d[1] = uy; d[2] = uz; d[3] = ga.x; d[4] = ga.y; d[5] = ga.z; d[6] = __int_as_float(i);
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
    // Twelve lanes own one row (the layout of the scattered row loads above): lane `piece` of a group its floats
    // 4 piece .. 4 piece + 3, i.e. 16-byte pieces of parameter and moment rows, five rows per wave instruction, whatever
    // gaps culling has left between the rows; a lane evaluates the basis once per row.  The moment loads of kAhead
    // trips are requested before the first of them is used.
    float *sh_p = const_cast<float *>(g.sh);
    const float *dirs = s_dir + wave_first * 7;
    constexpr int kPieces = (kRest + 3) / 4, kPer = 64 / kPieces, kIter = (64 + kPer - 1) / kPer, kAhead = 4;
    const int grp = lane / kPieces, piece = lane - grp * kPieces;
    const bool in_grp = grp < kPer;
    constexpr int kLast = kRest - 4 * (kPieces - 1);  // floats of a row's last piece (1..4)
    const int nval = piece == kPieces - 1 ? kLast : 4;
#pragma unroll 1
    for (int it0 = 0; it0 < kIter; it0 += kAhead) {
      float4 mq[kAhead], vq[kAhead];
      size_t at[kAhead];
#pragma unroll
      for (int u = 0; u < kAhead; ++u) {
        const int r = (it0 + u) * kPer + grp;
        mq[u] = vq[u] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        at[u] = 0;
        if (it0 + u < kIter && in_grp && r < rows) {
          at[u] = (size_t)__float_as_int(dirs[r * 7 + 6]) * kRest + 4 * piece;
          if (nval == 4) {
            mq[u] = __builtin_bit_cast(float4, *reinterpret_cast<const gs::f4u *>(ad.m_sh + at[u]));
            vq[u] = __builtin_bit_cast(float4, *reinterpret_cast<const gs::f4u *>(ad.v_sh + at[u]));
          } else {
            mq[u].x = ad.m_sh[at[u]]; vq[u].x = ad.v_sh[at[u]];
            if (nval > 1) { mq[u].y = ad.m_sh[at[u] + 1]; vq[u].y = ad.v_sh[at[u] + 1]; }
            if (nval > 2) { mq[u].z = ad.m_sh[at[u] + 2]; vq[u].z = ad.v_sh[at[u] + 2]; }
          }
        }
      }
#pragma unroll
      for (int u = 0; u < kAhead; ++u) {
        const int r = (it0 + u) * kPer + grp;
        if (it0 + u < kIter && in_grp && r < rows) {
          const float *d = dirs + r * 7;
          float Y[n];
          gs::sh_basis<L>(d[0], d[1], d[2], Y);
          const float *prow = wsh + r * kRest + 4 * piece;
          float pv[4] = {prow[0], nval > 1 ? prow[1] : 0.0f, nval > 2 ? prow[2] : 0.0f, nval > 3 ? prow[3] : 0.0f};
          float mv[4] = {mq[u].x, mq[u].y, mq[u].z, mq[u].w}, vv[4] = {vq[u].x, vq[u].y, vq[u].z, vq[u].w};
#pragma unroll
          for (int t = 0; t < 4; ++t) {
            if (t < nval) {
              const int c = 4 * piece + t, k = c / 3, ch = c - 3 * k;
              float yv = 0.0f;
#pragma unroll
              for (int q = 0; q < n - 1; ++q) yv = k == q ? Y[q + 1] : yv;
              const float grad = d[3 + ch] * yv;
              gs::adam_values(pv[t], mv[t], vv[t], grad, ad.lr_sh, ad.b1, ad.b2, ad.eps, ad.bias1, ad.bias2);
            }
          }
          if (nval == 4) {
            *reinterpret_cast<gs::f4u *>(sh_p + at[u]) = gs::f4u{pv[0], pv[1], pv[2], pv[3]};
            *reinterpret_cast<gs::f4u *>(ad.m_sh + at[u]) = gs::f4u{mv[0], mv[1], mv[2], mv[3]};
            *reinterpret_cast<gs::f4u *>(ad.v_sh + at[u]) = gs::f4u{vv[0], vv[1], vv[2], vv[3]};
          } else {
            for (int t = 0; t < nval; ++t) { sh_p[at[u] + t] = pv[t]; ad.m_sh[at[u] + t] = mv[t]; ad.v_sh[at[u] + t] = vv[t]; }
          }
        }
      }
    }
  }
  float gx = 0.0f, gy = 0.0f, gz = 0.0f, b0g[3] = {0.0f, 0.0f, 0.0f};
  const gs::Mat34 vw = gs::load_view(view);
  const gs::Mat44 pr = gs::load_proj(proj);
  const int jr = live ? j : jw;  // dead lanes of the last wave recompute row jw and store nothing
  const float4 a = rows_in[4 * jr], b = rows_in[4 * jr + 1], c = rows_in[4 * jr + 2];
  const float g_rgb[3] = {a.x, a.y, a.z};
  const float g_op = a.w;
  const float g_con[3] = {b.x, b.y, b.z};
  const float g_u = b.w, g_v = c.x;
  // the densification statistic's two components: the gradient's, or (kAbsRow) the absolute sums of slots 10 and 11
  const float n_u = kAbsRow ? c.z : g_u, n_v = kAbsRow ? c.w : g_v;
  if constexpr (kAdam == 3 && kRest > 0) {
    // gs::sh_bwd's two results from elsewhere: band 0's gradient is its own expression (Y_0 is the constant), the position
    // gradient through the view direction is what sh_adam_dir_kernel left (the same sums in the same order)
    b0g[0] = g_rgb[0] * GS_SH_C0; b0g[1] = g_rgb[1] * GS_SH_C0; b0g[2] = g_rgb[2] * GS_SH_C0;
    gx = ad.dir[3 * (size_t)jr]; gy = ad.dir[3 * (size_t)jr + 1]; gz = ad.dir[3 * (size_t)jr + 2];
  } else if constexpr (kDirSums) {
    // gs::sh_bwd without the row: its direction, its gradient expressions, and its last lines on the forward's sums
    float s[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) s[k] = dir_sums[9 * (size_t)jr + k];
    float ux, uy, uz, len;
    gs::view_dir(g.xyz[3 * i], g.xyz[3 * i + 1], g.xyz[3 * i + 2], cx, cy, cz, ux, uy, uz, len);
    float Y[n];
    gs::sh_basis<L>(ux, uy, uz, Y);
    b0g[0] = g_rgb[0] * Y[0]; b0g[1] = g_rgb[1] * Y[0]; b0g[2] = g_rgb[2] * Y[0];
    if constexpr (kAdam == 0) {  // (kAdam 1 stores no coefficient gradients: sh_bwd<L, false>)
      [[maybe_unused]] float *row = wsh + lane * kRest;
#pragma unroll
      for (int k = 0; k < n - 1; ++k) {
        const float yv = Y[k + 1];
        row[3 * k] = g_rgb[0] * yv; row[3 * k + 1] = g_rgb[1] * yv; row[3 * k + 2] = g_rgb[2] * yv;
      }
    }
    gs::sh_dir_finish(s, g_rgb, ux, uy, uz, len, gx, gy, gz);
  } else {
    float *row = wsh + lane * kRest;  // read as coefficients, overwritten with their gradients (kAdam: left as they are)
    gs::sh_bwd<L, kAdam == 0>(row, g.rgb + 3 * i, g.xyz[3 * i], g.xyz[3 * i + 1], g.xyz[3 * i + 2], cx, cy, cz, g_rgb, row, b0g,
                          gx, gy, gz);
  }
  if constexpr (kRest > 0 && kAdam == 0) {
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
    if (o.sh) gs::rows_from_lds<kRest>(o.sh + (size_t)jw * kRest, wsh, rows, lane);
  }
  if constexpr (!kCamGrad) {
    if (!live) return;
  }  // (kCamGrad: dead lanes go on with row jw's values, which they weigh 0 in the wave's sum, and store nothing)
  gx = 0.0f + gx; gy = 0.0f + gy; gz = 0.0f + gz;
  [[maybe_unused]] const float g_dir[3] = {gx, gy, gz};  // the position gradient through the view direction alone
  // kAdam: one three-vector group of this lane's gaussian: parameter and moments at the GLOBAL row i
  auto step3 = [&](const float *pc, float *m, float *v, const float *gr, float lr) {
    float *p = const_cast<float *>(pc);
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      float pv = p[3 * i + k], mv = m[3 * i + k], vv = v[3 * i + k];
      gs::adam_values(pv, mv, vv, gr[k], lr, ad.b1, ad.b2, ad.eps, ad.bias1, ad.bias2);
      p[3 * i + k] = pv; m[3 * i + k] = mv; v[3 * i + k] = vv;
    }
  };
  if constexpr (kAdam != 0) {
    // what is final already -- band 0 (nothing below reads it again), the opacity, the densification statistics
    // (cuda/trainer.cu:1136-1157, optimizer_step_kernel's expressions) -- leaves now, not across the covariance chain
    step3(g.rgb, ad.m_rgb, ad.v_rgb, b0g, ad.lr_rgb);
    {
      float pv = g.opacity[i], mv = ad.m_op[i], vv = ad.v_op[i];
      gs::adam_values(pv, mv, vv, g_op, ad.lr_op, ad.b1, ad.b2, ad.eps, ad.bias1, ad.bias2);
      const_cast<float *>(g.opacity)[i] = pv; ad.m_op[i] = mv; ad.v_op[i] = vv;
    }
    if (ad.uv_accum) ad.uv_accum[i] += sqrtf(n_u * n_u + n_v * n_v);
    if (ad.accum_dur) ad.accum_dur[i] += 1;
  }
  // conic -> (J, Sigma).  Sigma, J and the conic are RECOMPUTED from what this kernel reads anyway (quaternion, scale,
  // camera-space position) with the forward's functions and the forward's tan(fov): bit for bit the values
  // preprocess_kernel stored, without reading 60 bytes per gaussian back (the kernel is HBM bound).
  const int jc = kCamGrad ? jr : j;
  float x, y, z;
  if constexpr (kDirSums) {
    gs::camera_space(vw, g.xyz[3 * i], g.xyz[3 * i + 1], g.xyz[3 * i + 2], x, y, z);  // (as preprocess_kernel formed it)
  } else {
    x = xyz_c_sel[3 * jc]; y = xyz_c_sel[3 * jc + 1]; z = xyz_c_sel[3 * jc + 2];
  }
  float Jv[6], sg[6], con[3], rad_unused[4], dJ[6], dS[6];
  {
    const float4 q = reinterpret_cast<const float4 *>(g.quaternion)[i];
    const gs::RotScale rs = gs::rot_scale(q.x, q.y, q.z, q.w, g.scale[3 * i], g.scale[3 * i + 1], g.scale[3 * i + 2]);
    gs::sigma_from(rs, sg);
  }
  gs::jacobian(x, y, z, fx, fy, fwd_tan_fovx, fwd_tan_fovy, Jv);
  float dM[kCamGrad ? 6 : 1];
  [[maybe_unused]] float g_logit = g_op;  // what the opacity's gradient array gets (kAntialias: its share of g_eff)
  if constexpr (kAntialias) {
    float rho, cov_raw[3], drho, dcov[3];
    gs::conic_radius<true>(Jv, sg, vw, mh_dist, con, rad_unused, &rho, cov_raw);
    gs::effective_opacity_bwd(g_op, gs::sigmoid_fast(g.opacity[i]), rho, g_logit, drho);
    gs::compensation_bwd(cov_raw, rho, drho, dcov);
    gs::conic_bwd<false, true>(Jv, sg, vw, con, g_con, dJ, dS, nullptr, dcov);
  } else {
    gs::conic_radius(Jv, sg, vw, mh_dist, con, rad_unused);
    gs::conic_bwd<kCamGrad>(Jv, sg, vw, con, g_con, dJ, dS, dM);
  }
#pragma unroll
  for (int k = 0; k < 6; ++k) { dJ[k] = 0.0f + dJ[k]; dS[k] = 0.0f + dS[k]; }
  [[maybe_unused]] float jt_dm[kCamGrad ? 9 : 1];  // dL/dW through M = J W: (J^T dM)[r][c]
  if constexpr (kCamGrad) {
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
      for (int k = 0; k < 3; ++k) jt_dm[3 * r + k] = Jv[r] * dM[k] + Jv[3 + r] * dM[3 + k];
  }
  // J -> xyz_c
  float cxg, cyg, czg;
  gs::jacobian_bwd(x, y, z, fx, fy, tan_fovx, tan_fovy, dJ, cxg, cyg, czg);
  cxg = 0.0f + cxg; cyg = 0.0f + cyg; czg = 0.0f + czg;
  // Sigma -> quaternion, scale.  The rotation/scale terms are built a second time from a second (L2-resident) read
  // through an opaque copy of the index: kept alive across conic_bwd they cost 58 VGPRs and a third of the occupancy.
  int i2 = i;
  asm volatile("" : "+v"(i2));
  const float4 q = reinterpret_cast<const float4 *>(g.quaternion)[i2];
  const gs::RotScale rs = gs::rot_scale(q.x, q.y, q.z, q.w, g.scale[3 * i2], g.scale[3 * i2 + 1], g.scale[3 * i2 + 2]);
  float dQ[4], dSc[3];
  gs::sigma_bwd(rs, dS, dQ, dSc);
  // uv -> xyz_c
  float px_, py_, pz_;
  gs::to_screen_bwd(pr, x, y, z, g_u, g_v, width, height, px_, py_, pz_);
  cxg += px_; cyg += py_; czg += pz_;
  // depth mode: row slot 9 is dL/dz of the composited depth (render_bwd_kernel<.., kDepth>; gs_render.h: DepthMaps)
  if constexpr (kDepthRow) czg += c.y;
  // xyz_c -> xyz
  float wx, wy, wz;
  gs::camera_space_bwd(vw, cxg, cyg, czg, wx, wy, wz);
  gx += wx; gy += wy; gz += wz;
  if constexpr (kAdam != 0) {
    // the groups whose gradients the covariance chain produced: position (kAdam 2), scale, rotation
    if constexpr (kAdam == 2 || kAdam == 3) {
      const float gxyz[3] = {gx, gy, gz};
      step3(g.xyz, ad.m_xyz, ad.v_xyz, gxyz, ad.lr_xyz);
    }
    step3(g.scale, ad.m_sc, ad.v_sc, dSc, ad.lr_sc);
    {
      float4 pq = reinterpret_cast<const float4 *>(g.quaternion)[i];
      float4 mq = reinterpret_cast<const float4 *>(ad.m_q)[i], vq = reinterpret_cast<const float4 *>(ad.v_q)[i];
      gs::adam_values(pq.x, mq.x, vq.x, dQ[0], ad.lr_q, ad.b1, ad.b2, ad.eps, ad.bias1, ad.bias2);
      gs::adam_values(pq.y, mq.y, vq.y, dQ[1], ad.lr_q, ad.b1, ad.b2, ad.eps, ad.bias1, ad.bias2);
      gs::adam_values(pq.z, mq.z, vq.z, dQ[2], ad.lr_q, ad.b1, ad.b2, ad.eps, ad.bias1, ad.bias2);
      gs::adam_values(pq.w, mq.w, vq.w, dQ[3], ad.lr_q, ad.b1, ad.b2, ad.eps, ad.bias1, ad.bias2);
      reinterpret_cast<float4 *>(const_cast<float *>(g.quaternion))[i] = pq;
      reinterpret_cast<float4 *>(ad.m_q)[i] = mq; reinterpret_cast<float4 *>(ad.v_q)[i] = vq;
    }
    if (!o.xyz) return;  // (gradient arrays: only when the caller asked for them)
  }
  // stores (kCamGrad: live lanes only, and only when the caller gave arrays -- `out` may be NULL there)
  if (!kCamGrad || (live && o.xyz)) {
    if constexpr (kAdam == 1) {
      // what the optimizer kernels behind this one need: the position gradient and the colour gradient the SH gradients
      // are made of; the other arrays only where the caller gave them
      o.xyz[3 * j] = gx; o.xyz[3 * j + 1] = gy; o.xyz[3 * j + 2] = gz;
      if (o.opacity) o.opacity[j] = g_op;
      if (o.scale) { o.scale[3 * j] = dSc[0]; o.scale[3 * j + 1] = dSc[1]; o.scale[3 * j + 2] = dSc[2]; }
      if (o.quaternion) reinterpret_cast<float4 *>(o.quaternion)[j] = make_float4(dQ[0], dQ[1], dQ[2], dQ[3]);
    } else if (o.common) {  // the exchange's row, in global order (the same twelve values pack_split_kernel gathers)
      gs::f4u *row = reinterpret_cast<gs::f4u *>(o.common + (size_t)i * 12);
      row[0] = gs::f4u{gx, gy, gz, kAntialias ? g_logit : g_op};
      row[1] = gs::f4u{dSc[0], dSc[1], dSc[2], dQ[0]};
      row[2] = gs::f4u{dQ[1], dQ[2], dQ[3], 1.0f};
      if (o.uv_norm) o.uv_norm[i] = sqrtf(n_u * n_u + n_v * n_v);  // pack_uv_norm_kernel's expression
    } else {
      o.xyz[3 * j] = gx; o.xyz[3 * j + 1] = gy; o.xyz[3 * j + 2] = gz;
      o.opacity[j] = kAntialias ? g_logit : g_op;
      o.scale[3 * j] = dSc[0]; o.scale[3 * j + 1] = dSc[1]; o.scale[3 * j + 2] = dSc[2];
      reinterpret_cast<float4 *>(o.quaternion)[j] = make_float4(dQ[0], dQ[1], dQ[2], dQ[3]);
    }
    if (o.rgb) { o.rgb[3 * j] = b0g[0]; o.rgb[3 * j + 1] = b0g[1]; o.rgb[3 * j + 2] = b0g[2]; }
    if (o.conic) { o.conic[3 * j] = g_con[0]; o.conic[3 * j + 1] = g_con[1]; o.conic[3 * j + 2] = g_con[2]; }
    if (o.uv) { o.uv[2 * j] = g_u; o.uv[2 * j + 1] = g_v; }
    if (o.pre_rgb) { o.pre_rgb[3 * j] = g_rgb[0]; o.pre_rgb[3 * j + 1] = g_rgb[1]; o.pre_rgb[3 * j + 2] = g_rgb[2]; }
    if (o.J) {
#pragma unroll
      for (int k = 0; k < 6; ++k) o.J[6 * j + k] = dJ[k];
    }
    if (o.sigma) {
#pragma unroll
      for (int k = 0; k < 6; ++k) o.sigma[6 * j + k] = dS[k];
    }
    if (o.xyz_c) { o.xyz_c[3 * j] = cxg; o.xyz_c[3 * j + 1] = cyg; o.xyz_c[3 * j + 2] = czg; }
  }
  if constexpr (kCamGrad) {
    // This lane's share, in double: view[4r + c] += c_r p_c + (J^T dM)[r][c], view[4r + 3] += c_r, campos -= s, with
    // c = dL/d xyz_c (cxg..: Jacobian, screen and depth terms), p the world position, s the view-direction term.  Dead
    // lanes add exact zeros (a select, not a product: their row-jw values may be anything).  Then a fixed xor
    // butterfly over the wave that halves what a lane carries at every step (lane bit 5 keeps sums 0-7 or 8-15, bit 4
    // four of those, ...): 8 + 4 + 2 + 1 + 1 + 1 exchanges instead of 15 per step, and sum k = lane >> 2 ends in the
    // quad of lanes 4k..4k+3 -- the same bits in every run.
    const double p[3] = {g.xyz[3 * i], g.xyz[3 * i + 1], g.xyz[3 * i + 2]};
    const double cv[3] = {cxg, cyg, czg};
    double v[16];
#pragma unroll
    for (int r = 0; r < 3; ++r) {
#pragma unroll
      for (int k = 0; k < 3; ++k) v[4 * r + k] = live ? cv[r] * p[k] + (double)jt_dm[3 * r + k] : 0.0;
      v[4 * r + 3] = live ? cv[r] : 0.0;
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) v[12 + k] = live ? -(double)g_dir[k] : 0.0;
    v[15] = 0.0;
#pragma unroll
    for (int half = 8, bit = 32; half >= 1; half >>= 1, bit >>= 1) {
      const bool upper = (lane & bit) != 0;
#pragma unroll
      for (int k = 0; k < half; ++k) {
        const double send = upper ? v[k] : v[k + half], keep = upper ? v[k + half] : v[k];
        v[k] = keep + __shfl_xor(send, bit, 64);
      }
    }
    v[0] += __shfl_xor(v[0], 2, 64);
    v[0] += __shfl_xor(v[0], 1, 64);
    if ((lane & 3) == 0) cam_rows[(size_t)(jw >> 6) * 16 + (lane >> 2)] = v[0];  // (sum 15 is the zero pad)
  }
}

// kCamGrad's second half: one workgroup sums the waves' rows in a fixed order -- thread t the component pair t & 7 of
// rows t >> 3, (t >> 3) + 128, ..., then a tree over the 128 partial rows in LDS -- in double, and overwrites the fifteen
// float results.  No atomics and no hand-off between workgroups: the same bits in every run.
constexpr int kCamFinThreads = 1024;
__global__ __launch_bounds__(kCamFinThreads) void cam_grad_finalize_kernel(const double *__restrict__ rows, int n_rows,
                                                                           float *__restrict__ grad_view,
                                                                           float *__restrict__ grad_campos) {
  constexpr int kSlots = kCamFinThreads / 8;
  __shared__ double2 s_part[kCamFinThreads];
  const int t = threadIdx.x, piece = t & 7;
  const double2 *r2 = reinterpret_cast<const double2 *>(rows);
  double2 acc = make_double2(0.0, 0.0);
#pragma unroll 8
  for (int r = t >> 3; r < n_rows; r += kSlots) {
    const double2 v = r2[(size_t)r * 8 + piece];
    acc.x += v.x;
    acc.y += v.y;
  }
  s_part[t] = acc;
  __syncthreads();
  for (int half = kCamFinThreads / 2; half >= 8; half >>= 1) {  // (half is a multiple of 8: partners share a piece)
    if (t < half) {
      const double2 o = s_part[t + half];
      s_part[t].x += o.x;
      s_part[t].y += o.y;
    }
    __syncthreads();
  }
  if (t < 8) {
    const double2 v = s_part[t];
    const double pair[2] = {v.x, v.y};
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int k = 2 * t + h;
      if (k < 12) grad_view[k] = (float)pair[h];
      else if (k < 15) grad_campos[k - 12] = (float)pair[h];
    }
  }
}

// r06 (gsplat_adam_fused.mode 2): the SH group's Adam step and gs::sh_bwd's sums over the coefficient rows in ONE read of
// the rows.  The unfused iteration reads them twice -- preprocess_bwd_kernel for d colour / d direction, then
// optimizer_sh_factored_kernel for the update -- and the one fat kernel (kAdam 2) reads them once but at three waves per
// SIMD.  Here sixteen lanes own one gaussian: lane k its coefficient k + 1 (three channels: 12 bytes of the parameter row
// and of both moment rows, neighbouring lanes neighbouring pieces, as optimizer_sh_factored_kernel).  Every lane evaluates
// the basis and its gradient at the row's direction and keeps its own coefficient's entries; the update is
// optimizer_sh_factored_kernel's (gradient = g_rgb[channel] * Y_k), from the OLD coefficients the lane also forms its
// nine products dY_k/d(axis) * coefficient[channel], and the nine sums over k run through the row as a chain of DPP adds
// (row_shr:1, one instruction per step and sum): lane k ends with exactly gs::sh_bwd's left-to-right partial sum
// ((0 + band-0 term) + k = 1) + ... + k, so the
// last coefficient's lane holds sh_bwd's sums BIT FOR BIT and finishes its three outputs.  No LDS, ~60 registers.
template <int L>
__global__ __launch_bounds__(kBlock) void sh_adam_dir_kernel(int M, const int *__restrict__ c2g, float *__restrict__ sh,
                                                             float *__restrict__ m, float *__restrict__ v, float lr,
                                                             float b1, float b2, float eps, float bias1, float bias2,
                                                             const float *__restrict__ xyz,
                                                             const float *__restrict__ band0, float cx, float cy, float cz,
                                                             const float4 *__restrict__ rows_in, float *__restrict__ dir_out) {
  constexpr int n = (L + 1) * (L + 1), kCoef = n - 1;
  static_assert(L >= 1 && kCoef <= 15, "one 16-lane row per gaussian");
  const unsigned int t = blockIdx.x * (unsigned int)kBlock + threadIdx.x;
  const unsigned int r = t >> 4;
  const int k = (int)(t & 15u);
  if (r >= (unsigned int)M) return;  // (a whole DPP row leaves together)
  const long long row = c2g[r];
  const float4 ga = rows_in[4 * (size_t)r];  // d loss / d colour of this view: rows[.][0..2]
  const float gr[3] = {ga.x, ga.y, ga.z};
  float ux, uy, uz, len;
  gs::view_dir(xyz[3 * row], xyz[3 * row + 1], xyz[3 * row + 2], cx, cy, cz, ux, uy, uz, len);
  float Y[n], dY[n][3];
  gs::sh_basis<L>(ux, uy, uz, Y);
  gs::sh_basis_grad<L>(ux, uy, uz, dY);
  float yv = 0.0f, dd[3] = {0.0f, 0.0f, 0.0f};
#pragma unroll
  for (int q = 0; q < kCoef; ++q) {
    yv = k == q ? Y[q + 1] : yv;
    dd[0] = k == q ? dY[q + 1][0] : dd[0]; dd[1] = k == q ? dY[q + 1][1] : dd[1]; dd[2] = k == q ? dY[q + 1][2] : dd[2];
  }
  const bool act = k < kCoef;
  const long long o = (row * kCoef + k) * 3;
  float p[3] = {0.0f, 0.0f, 0.0f};
  if (act) {
    float mm[3], vv[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) { p[c] = sh[o + c]; mm[c] = m[o + c]; vv[c] = v[o + c]; }
    float pn[3] = {p[0], p[1], p[2]};
#pragma unroll
    for (int c = 0; c < 3; ++c) gs::adam_values(pn[c], mm[c], vv[c], gr[c] * yv, lr, b1, b2, eps, bias1, bias2);
#pragma unroll
    for (int c = 0; c < 3; ++c) { sh[o + c] = pn[c]; m[o + c] = mm[c]; v[o + c] = vv[c]; }
  }
  // acc[axis][channel]: gs::sh_bwd's dRx dGx dBx | dRy .. | dRz ..  x = what a lane adds: its product, in lane 0 sh_bwd's
  // start (0 + band-0 term) + product.  One DPP add per step and sum: lane l takes lane l - 1's partial sum + x; lane 0 gets a
  // zero shifted in and re-forms 0 + x = its start (never -0: a sum that began with + 0 is not), so there is no select.
  float x[3][3], acc[3][3];
#pragma unroll
  for (int a = 0; a < 3; ++a)
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const float leaf = dd[a] * p[c];
      float first = 0.0f;
      first += dY[0][a] * band0[3 * row + c];
      first += leaf;
      x[a][c] = acc[a][c] = k == 0 ? first : leaf;
    }
#pragma unroll
  for (int step = 1; step < kCoef; ++step)
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
      for (int c = 0; c < 3; ++c)
        acc[a][c] = __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(acc[a][c]), 0x111 /* row_shr:1 */, 0xF, 0xF, true)) + x[a][c];
  if (k == kCoef - 1) {  // gs::sh_bwd's last lines
    const float tx = gr[0] * acc[0][0] + gr[1] * acc[0][1] + gr[2] * acc[0][2];
    const float ty = gr[0] * acc[1][0] + gr[1] * acc[1][1] + gr[2] * acc[1][2];
    const float tz = gr[0] * acc[2][0] + gr[1] * acc[2][1] + gr[2] * acc[2][2];
    const float dot = tx * ux + ty * uy + tz * uz;
    dir_out[3 * (size_t)r] = (tx - dot * ux) / len;
    dir_out[3 * (size_t)r + 1] = (ty - dot * uy) / len;
    dir_out[3 * (size_t)r + 2] = (tz - dot * uz) / len;
  }
}

}  // namespace

namespace gs {

// The instantiations are exactly these: (L 0..3) x (depth row) x { the camera form | (abs row) x { kAdam 1, 2, 3 | the
// anti-aliased form | the plain form } } -- the camera form stores no statistic and has no kAbsRow instantiation, the
// anti-aliased form exists only for kAdam == 0 without the camera gradient (the kernel's static_asserts); the plain form
// and kAdam 1 also as kDirSums
int launch_preprocess_bwd(const PreprocessBwdArgs &a, hipStream_t st) {
  GS_REQUIRE(a.span > 0, "nothing to launch");
  GS_REQUIRE(a.adam_mode >= 0 && a.adam_mode <= 3 && (a.adam_mode == 0 || a.adam != nullptr), "bad Adam form");
  GS_REQUIRE(!a.cam_rows || (a.adam_mode == 0 && !a.antialiased), "the camera gradient is a form of the plain backward");
  GS_REQUIRE(!a.antialiased || a.adam_mode == 0, "anti-aliased mode is a form of the plain backward");
  GS_REQUIRE(!a.dir_sums || (a.adam_mode <= 1 && !a.cam_rows && !a.antialiased),
             "the direction sums are read by the plain form and by adam_mode 1 only");
  const gsplat_gradients &g = a.out;
  const BwdOut o = {g.grad_xyz, g.grad_rgb, g.grad_sh, g.grad_opacity, g.grad_scale, g.grad_quaternion, g.grad_conic,
                    g.grad_uv, g.grad_J, g.grad_sigma, g.grad_xyz_c, g.grad_precompute_rgb, a.common, a.uv_norm};
  AdamFused ad = {};  // (value-initialised: every pointer null)
  if (a.adam_mode) {
    const gsplat_adam_fused &p = *a.adam;
    ad = {p.exp_avg[0], p.exp_avg_sq[0], p.exp_avg[1], p.exp_avg_sq[1], p.exp_avg[2], p.exp_avg_sq[2],
          p.exp_avg[3], p.exp_avg_sq[3], p.exp_avg[4], p.exp_avg_sq[4], p.exp_avg[5], p.exp_avg_sq[5],
          p.lr[0], p.lr[1], p.lr[2], p.lr[3], p.lr[4], p.lr[5],
          p.b1, p.b2, p.eps, p.bias1, p.bias2, p.uv_grad_accum, p.grad_accum_dur, a.adam_dir};
  }
  const dim3 grid(div_up(a.span, kBlock)), block(kBlock);
  auto launch = [&](auto kernel) {
    kernel<<<grid, block, 0, st>>>(a.g, a.view, a.proj, a.M, a.c2g, a.xyz_c, a.rows, a.fx, a.fy, a.tan_fovx, a.tan_fovy,
                                   a.fwd_tan_fovx, a.fwd_tan_fovy, a.mh_dist, a.campos[0], a.campos[1], a.campos[2], a.width,
                                   a.height, o, a.ranged, a.first, a.end, ad, a.cam_rows, a.dir_sums);
  };
  with_degree<0>(a.l_max, [&](auto L) {
    with_bool(a.rows_depth, [&](auto dr) {
      constexpr int kL = decltype(L)::value;
      constexpr bool kDR = decltype(dr)::value;
      if (a.cam_rows) return launch(preprocess_bwd_kernel<kL, 0, kDR, true>);
      with_bool(a.rows_abs, [&](auto ab) {
        constexpr bool kAB = decltype(ab)::value;
        if (a.adam_mode == 1 && a.dir_sums) launch(preprocess_bwd_kernel<kL, 1, kDR, false, kAB, false, true>);
        else if (a.adam_mode == 1) launch(preprocess_bwd_kernel<kL, 1, kDR, false, kAB>);
        else if (a.adam_mode == 3) launch(preprocess_bwd_kernel<kL, 3, kDR, false, kAB>);
        else if (a.adam_mode) launch(preprocess_bwd_kernel<kL, 2, kDR, false, kAB>);
        else if (a.antialiased) launch(preprocess_bwd_kernel<kL, 0, kDR, false, kAB, true>);
        else if (a.dir_sums) launch(preprocess_bwd_kernel<kL, 0, kDR, false, kAB, false, true>);
        else launch(preprocess_bwd_kernel<kL, 0, kDR, false, kAB>);
      });
    });
  });
  GS_LAUNCH_CHECK();
  if (a.cam_rows) {
    cam_grad_finalize_kernel<<<1, kCamFinThreads, 0, st>>>(a.cam_rows, (int)div_up(a.span, 64), a.grad_view, a.grad_campos);
    GS_LAUNCH_CHECK();
  }
  return GSPLAT_OK;
}

int launch_sh_adam_dir(const ShAdamDirArgs &a, hipStream_t st) {
  GS_REQUIRE(a.l_max >= 1 && a.M > 0, "degree 0 has no SH group; nothing to launch for M = 0");
  const unsigned int blocks = (unsigned int)(((long long)a.M * 16 + kBlock - 1) / kBlock);
  with_degree<1>(a.l_max, [&](auto L) {
    sh_adam_dir_kernel<decltype(L)::value><<<blocks, kBlock, 0, st>>>(a.M, a.c2g, a.sh, a.m, a.v, a.lr, a.b1, a.b2, a.eps, a.bias1,
                                                                      a.bias2, a.xyz, a.band0, a.campos[0], a.campos[1],
                                                                      a.campos[2], a.rows, a.dir_out);
  });
  GS_LAUNCH_CHECK();
  return GSPLAT_OK;
}

}  // namespace gs
