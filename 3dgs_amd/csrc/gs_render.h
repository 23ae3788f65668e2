// gs_render.h -- device helpers shared by the compositing kernels (gs_render_fwd.hip, gs_render_bwd.hip), the kernels
// that replay a recorded forward (gs_replay.hip) and the fused preprocess kernel (gs_preprocess.hip): the 48-byte
// "splat record" a tile stages in LDS, wave64 cross-lane reductions on DPP, the XCD-aware block -> tile map, the
// launchers' argument structs, and the batch staging and row lists of the tile walk.
#pragma once
#include <hip/hip_ext.h>
#include <hip/hip_runtime.h>

#include <type_traits>

namespace gs {

constexpr float kAlphaMin = 0.00392156862f;  // 1/255, cuda/render.cu:74
constexpr float kAlphaMax = 0.99f;           // cuda/render.cu:73
constexpr float kTMin = 0.0001f;             // cuda/render.cu:77
// log2(0.99) = -0.01449957, minus two ulps of a value near one under exp2: the forward's cap in the exponent domain
// (render_fwd_kernel staging) -- v_exp_f32 of it is at most 0.99f
constexpr float kLog2AlphaMax = -0.01449975f;

// Everything the compositing loops need about one gaussian, as three float4:
//   r0 = {u, v, conic00, conic01}
//   r1 = {conic11, sigmoid(opacity), hx, hy}   hx/hy: half extents of the axis-aligned box that
//                                              contains every pixel centre with alpha >= 1/255
//   r2 = {r, g, b, <16 block-hit bits, filled per tile>}
struct SplatRec { float4 r0, r1, r2; };

__device__ __forceinline__ float sigmoid_fast(float logit) { return 1.0f / (1.0f + __expf(-logit)); }

// Conservative footprint: alpha = min(.99, opa*exp(p)) can reach 1/255 only where
// p >= -tau, tau = ln(255*opa), i.e. inside the ellipse 0.5 d^T C d <= tau, whose bounding
// box has half widths sqrt(2 tau C^-1_xx), sqrt(2 tau C^-1_yy).  Degenerate / NaN conics
// get an infinite box (always visited), opacities that can never reach 1/255 an empty one.
// Returns tau2 = 2 tau (+ margin), the level of the quadratic form a dx^2 + 2 b dx dy + c dy^2 at that ellipse.
__device__ __forceinline__ float footprint(float a, float b, float c, float opa, float &hx, float &hy) {
  const float det = a * c - b * b;
  if (!(opa * 255.0f >= 0.999f)) {
    hx = hy = -INFINITY;
    if (opa != opa) hx = hy = INFINITY;
    return 0.0f;
  }
  if (!(det > 0.0f) || !(a > 0.0f) || !(c > 0.0f) || !(det < INFINITY)) {
    hx = hy = INFINITY;
    return INFINITY;
  }
  const float tau2 = 2.0f * fmaxf(0.0f, logf(255.0f * opa)) + 1e-3f;
  hx = sqrtf(tau2 * c / det) * 1.0005f + 0.01f;
  hy = sqrtf(tau2 * a / det) * 1.0005f + 0.01f;
  return tau2;
}

// make_record on an opacity that is already a probability: the anti-aliased forward hands in sigmoid(logit) * rho
// (gsplat_context_set_antialiased), and everything the record derives from the opacity follows it
__device__ __forceinline__ SplatRec make_record_opa(float u, float v, float a, float b, float c, float opa, float r,
                                                    float g, float bl) {
  SplatRec s;
  float hx, hy;
  const float tau2 = footprint(a, b, c, opa, hx, hy);
  s.r0 = make_float4(u, v, a, b);
  s.r1 = make_float4(c, opa, hx, hy);
  s.r2 = make_float4(r, g, bl, tau2);
  return s;
}

__device__ __forceinline__ SplatRec make_record(float u, float v, float a, float b, float c, float logit, float r,
                                                float g, float bl) {
  return make_record_opa(u, v, a, b, c, sigmoid_fast(logit), r, g, bl);
}

// 16-bit mask: bit (4*by + bx) set when the ellipse alpha >= 1/255 may touch the 4x4 pixel block (bx, by) of the tile
// whose first pixel is (x0, y0) -- the ellipse itself, not its bounding box.  For each of the tile's four strips of pixel rows (dy in [Y0, Y0+3]
// about the centre) the ellipse q(dx, dy) = a dx^2 + 2 b dx dy + c dy^2 <= tau2 covers the dx-interval
// [min_y L(y), max_y R(y)], L/R(y) = -(b/a) y -/+ sqrt((tau2 - (det/a) y^2) / a); R is concave with its maximum at the
// dy of the ellipse's rightmost point, -(b/c) hx, L convex with its minimum at +(b/c) hx, so each bound is one
// evaluation at that dy clamped into the strip: two square roots per strip, about 200 instructions per (gaussian,
// tile) -- once, the forward hands the masks to the backward.  On the benchmark scene the box admits 17.4 M
// (gaussian, block) pairs, the ellipse 14.3 M: 17 % fewer loop trips in both compositing kernels.  Degenerate conics
// (infinite box) visit every block; what a NaN centre visits does not matter (its alpha is NaN on every pixel: no splat).
__device__ __forceinline__ unsigned int block_hits(const SplatRec &s, float x0, float y0) {
  const float a = s.r0.z, b = s.r0.w, c = s.r1.x, hx = s.r1.z, hy = s.r1.w, tau2 = s.r2.w;
  if (!(hx < INFINITY) || !(hy < INFINITY)) return 0xFFFFu;  // degenerate conic or NaN: always visited
  if (!(hx > 0.0f)) return 0u;                                // opacity can never reach 1/255
  const float inv_a = 1.0f / a, boa = b * inv_a;
  const float kappa = c - b * boa;    // det / a
  const float ystar = -(b / c) * hx;  // dy of the rightmost point; the leftmost one sits at -ystar
  const float U = s.r0.x - x0, V = s.r0.y - y0;  // centre relative to the tile's first pixel
  unsigned int out = 0u;
#pragma unroll 1  // one strip at a time: unrolled, the four strips' temporaries push the callers past their VGPR step
  for (int l = 0; l < 4; ++l) {
    const float Y0 = 4.0f * (float)l - V, Y1 = Y0 + 3.0f;
    const float ylo = fmaxf(Y0, -hy), yhi = fminf(Y1, hy);
    const float yr = __builtin_amdgcn_fmed3f(ystar, ylo, yhi), yl = __builtin_amdgcn_fmed3f(-ystar, ylo, yhi);
    const float wr = __builtin_sqrtf(fmaxf(0.0f, (tau2 - kappa * yr * yr) * inv_a));
    const float wl = __builtin_sqrtf(fmaxf(0.0f, (tau2 - kappa * yl * yl) * inv_a));
    const float R = wr - boa * yr, L = -wl - boa * yl;
    const float Rm = R + (0.01f + 5e-4f * fabsf(R)), Lm = L - (0.01f + 5e-4f * fabsf(L));
    // blocks k with 4k - U <= Rm and 4k + 3 - U >= Lm: k in [ceil((Lm + U - 3) / 4), floor((Rm + U) / 4)]
    const int k_hi = min(3, (int)floorf((Rm + U) * 0.25f)), k_lo = max(0, (int)ceilf((Lm + U - 3.0f) * 0.25f));
    unsigned int row = k_hi >= k_lo ? ((2u << k_hi) - (1u << k_lo)) : 0u;
    if (ylo > yhi) row = 0u;  // the strip lies above or below the ellipse
    out |= row << (4 * l);
  }
  return out;
}

// ---- staged (LDS) form of a record.  The compositing loops evaluate opa * exp(min(0, power)) as one base-2
// exponential with the opacity folded into the exponent,
//   log2(opa * exp(power)) = a2 dx^2 + b2 dx dy + c2 dy^2 + log2(opa),   (a2, b2, c2) = -log2(e) * (a/2, b, c/2),
// which takes four VALU instructions fewer per (pixel, gaussian) than power -> * log2(e) -> exp -> * opa.
// r0 = (u, v, a2, b2), r1 = (c2, log2 opa, opa, hy), r2 = (rgb, hit mask).  Both directions use the same form, so
// the backward recomputes the forward's alpha bit for bit.
constexpr float kLog2e = 1.44269504088896340736f;

__device__ __forceinline__ void stage_record(SplatRec &s) {
  const float opa = s.r1.y;
  s.r0.z *= -0.5f * kLog2e;
  s.r0.w *= -kLog2e;
  s.r1.x *= -0.5f * kLog2e;
  s.r1.y = __log2f(opa);  // -inf for opacity 0: alpha 0
  s.r1.z = opa;
}

// the all-zero sentinel record a list is padded with: alpha = 2^-inf = 0 at every pixel
__device__ __forceinline__ float4 sentinel_r1() { return make_float4(0.0f, -INFINITY, 0.0f, 0.0f); }

// log2 of the unclamped alpha; min(.., log2 opa) is the reference's min(0, power)
__device__ __forceinline__ float log2_alpha(float a2, float b2, float c2, float lopa, float dx, float dy) {
  float t = a2 * dx;
  t = __builtin_fmaf(b2, dy, t);
  float q;  // three-operand form on purpose: as v_fmac the compiler first copies lopa (still needed for the min)
  asm("v_fma_f32 %0, %1, %2, %3" : "=v"(q) : "v"(t), "v"(dx), "v"(lopa));
  q = __builtin_fmaf(c2 * dy, dy, q);
  float r;  // fminf() would first canonicalise the loaded lopa (one more VALU instruction per evaluation)
  asm("v_min_f32 %0, %1, %2" : "=v"(r) : "v"(q), "v"(lopa));
  return r;
}

// the forward's form: the clamp is min(log2 opa, log2 0.99) (staged per gaussian), so the result is the CAPPED alpha
__device__ __forceinline__ float staged_alpha_capped(float a2, float b2, float c2, float lopa, float lbound, float dx, float dy) {
  float t = a2 * dx;
  t = __builtin_fmaf(b2, dy, t);
  float q = __builtin_fmaf(t, dx, lopa);  // (lopa dies here: a plain v_fmac, no copy -- and no asm, whose borders cost a wait state)
  q = __builtin_fmaf(c2 * dy, dy, q);
  float r;
  asm("v_min_f32 %0, %1, %2" : "=v"(r) : "v"(q), "v"(lbound));
  return __builtin_amdgcn_exp2f(r);
}

// the conic entries back from their staged form (flush of the backward): a = a2 * kConicDiag, b = b2 * kConicOff
constexpr float kConicDiag = -2.0f / kLog2e, kConicOff = -1.0f / kLog2e;

// opa * exp(min(0, power)) from a staged record
__device__ __forceinline__ float staged_alpha(float a2, float b2, float c2, float lopa, float dx, float dy) {
  return __builtin_amdgcn_exp2f(log2_alpha(a2, b2, c2, lopa, dx, dy));
}

// ---- DPP helpers
template <int kCtrl>
__device__ __forceinline__ float dpp_add(float v) {
  const int moved = __builtin_amdgcn_update_dpp(0, __float_as_int(v), kCtrl, 0xF, 0xF, false);
  return v + __int_as_float(moved);
}
template <int kCtrl>
__device__ __forceinline__ float dpp_take(float v) {
  return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), kCtrl, 0xF, 0xF, false));
}
__device__ __forceinline__ float row_sum(float v) {  // every lane of a 16-lane row ends with the row total
  v = dpp_add<0xB1>(v);   // quad_perm [1,0,3,2]
  v = dpp_add<0x4E>(v);   // quad_perm [2,3,0,1]
  v = dpp_add<0x141>(v);  // row_half_mirror
  v = dpp_add<0x140>(v);  // row_mirror
  return v;
}
// ---- row-level (16 lanes) reduction of NINE values at once, for kernels where every 16-lane row works on its own
// (gaussian, 4x4 pixel block) pair.  Transposed butterfly: the two stages that pair lanes 4 and 8 apart fold two
// registers into one with TWO full-rate DPP adds (the second writes only the banks = 4-lane groups that keep the
// other value, via bank_mask), the two stages inside a quad use a select pair + one DPP add.  21 VALU, no
// v_permlane, and the nine row totals end up in nine different lanes of ONE register, so one ds_add_f32 adds
// all of them.  Lane j of a row (bits b3 b2 b1 b0): b1 == 0 -> total of value 4*b0 + 2*b3 + b2; b1 == 1 -> value 8.
// The block schedules its own DPP hazards (a VGPR written by VALU may be read by a DPP source operand only two
// instructions later): the leading s_nop covers the inputs, the ordering covers the rest.
__device__ __forceinline__ float row_sum9(float v0, float v1, float v2, float v3, float v4, float v5, float v6,
                                          float v7, float v8) {
  float r0, r1, r2, r3, r4, q0, q1, q2, snd, kp, m0, out;
  const unsigned long long odd = 0xAAAAAAAAAAAAAAAAull, bit1 = 0xCCCCCCCCCCCCCCCCull;
  asm volatile(
      "s_nop 1\n\t"
      // stage A: lanes 4 apart (lane bit 2): banks 0,2 keep the even value, banks 1,3 the odd one
      "v_add_f32_dpp %[r0], %[v0], %[v0] row_shl:4 row_mask:0xf bank_mask:0xf bound_ctrl:0\n\t"
      "v_add_f32_dpp %[r0], %[v1], %[v1] row_shr:4 row_mask:0xf bank_mask:0xa bound_ctrl:0\n\t"
      "v_add_f32_dpp %[r1], %[v2], %[v2] row_shl:4 row_mask:0xf bank_mask:0xf bound_ctrl:0\n\t"
      "v_add_f32_dpp %[r1], %[v3], %[v3] row_shr:4 row_mask:0xf bank_mask:0xa bound_ctrl:0\n\t"
      "v_add_f32_dpp %[r2], %[v4], %[v4] row_shl:4 row_mask:0xf bank_mask:0xf bound_ctrl:0\n\t"
      "v_add_f32_dpp %[r2], %[v5], %[v5] row_shr:4 row_mask:0xf bank_mask:0xa bound_ctrl:0\n\t"
      "v_add_f32_dpp %[r3], %[v6], %[v6] row_shl:4 row_mask:0xf bank_mask:0xf bound_ctrl:0\n\t"
      "v_add_f32_dpp %[r3], %[v7], %[v7] row_shr:4 row_mask:0xf bank_mask:0xa bound_ctrl:0\n\t"
      "v_add_f32_dpp %[r4], %[v8], %[v8] row_shl:4 row_mask:0xf bank_mask:0xf bound_ctrl:0\n\t"
      "v_add_f32_dpp %[r4], %[v8], %[v8] row_shr:4 row_mask:0xf bank_mask:0xa bound_ctrl:0\n\t"
      // stage B: lanes 8 apart (lane bit 3): banks 0,1 keep the even register, banks 2,3 the odd one
      "v_add_f32_dpp %[q0], %[r0], %[r0] row_shl:8 row_mask:0xf bank_mask:0xf bound_ctrl:0\n\t"
      "v_add_f32_dpp %[q0], %[r1], %[r1] row_shr:8 row_mask:0xf bank_mask:0xc bound_ctrl:0\n\t"
      "v_add_f32_dpp %[q1], %[r2], %[r2] row_shl:8 row_mask:0xf bank_mask:0xf bound_ctrl:0\n\t"
      "v_add_f32_dpp %[q1], %[r3], %[r3] row_shr:8 row_mask:0xf bank_mask:0xc bound_ctrl:0\n\t"
      "v_add_f32_dpp %[q2], %[r4], %[r4] row_shl:8 row_mask:0xf bank_mask:0xf bound_ctrl:0\n\t"
      "v_add_f32_dpp %[q2], %[r4], %[r4] row_shr:8 row_mask:0xf bank_mask:0xc bound_ctrl:0\n\t"
      // stage C: lane bit 0: even lanes keep q0, odd lanes q1; q2 is summed in place
      "v_cndmask_b32_e64 %[snd], %[q1], %[q0], %[odd]\n\t"
      "v_cndmask_b32_e64 %[kp], %[q0], %[q1], %[odd]\n\t"
      "s_nop 0\n\t"
      "v_add_f32_dpp %[r0], %[q2], %[q2] quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf\n\t"
      "v_add_f32_dpp %[m0], %[snd], %[kp] quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf\n\t"
      // stage D: lane bit 1: lanes with the bit clear keep m0 (values 0..7), the others value 8
      "v_cndmask_b32_e64 %[snd], %[r0], %[m0], %[bit1]\n\t"
      "v_cndmask_b32_e64 %[kp], %[m0], %[r0], %[bit1]\n\t"
      "s_nop 1\n\t"
      "v_add_f32_dpp %[out], %[snd], %[kp] quad_perm:[2,3,0,1] row_mask:0xf bank_mask:0xf\n\t"
      : [r0] "=&v"(r0), [r1] "=&v"(r1), [r2] "=&v"(r2), [r3] "=&v"(r3), [r4] "=&v"(r4), [q0] "=&v"(q0),
        [q1] "=&v"(q1), [q2] "=&v"(q2), [snd] "=&v"(snd), [kp] "=&v"(kp), [m0] "=&v"(m0), [out] "=&v"(out)
      : [v0] "v"(v0), [v1] "v"(v1), [v2] "v"(v2), [v3] "v"(v3), [v4] "v"(v4), [v5] "v"(v5), [v6] "v"(v6),
        [v7] "v"(v7), [v8] "v"(v8), [odd] "s"(odd), [bit1] "s"(bit1));
  return out;
}
__device__ __host__ __forceinline__ int row_sum9_index(int lane) {
  return (lane & 2) ? 8 : 4 * (lane & 1) + 2 * ((lane >> 3) & 1) + ((lane >> 2) & 1);
}
__device__ __host__ __forceinline__ bool row_sum9_active(int lane) { return !(lane & 2) || (lane & 15) == 2; }

// ---- the backward's nine row sums, products included.  Every sum is (a per-pixel factor) x (a lane constant):
//   rgb_c = sum aT * grad_c(pixel),   S_m = sum gp * m(cx, cy),  m in {1, cx, cy, cx^2, cx cy, cy^2},
// with (cx, cy) the pixel's position relative to the TILE centre (the moments about the gaussian's own centre follow
// per gaussian at flush time: dx = X - cx with X = u - tile centre).  So the first butterfly stage needs no separate
// products: with the partner lane l ^ 7 (row_half_mirror, which also swaps the two banks of a pair) a register of the
// stage is  F * W_own + dpp(F) * W_partner  = one v_mul + one v_fmac_dpp, W_* loop-invariant per lane.
// Ten instructions instead of nine products + ten adds.  Later stages as in row_sum9.
struct RowWeights {  // banks 0,2 (lane bit 2 clear) | banks 1,3
  float a_own, a_par;  // grad0 | grad1          x aT
  float b_own, b_par;  // grad2 | (unused)       x aT
  float c_own, c_par;  // 1     | cx             x gp
  float d_own, d_par;  // cy    | cx^2           x gp
  float e_own, e_par;  // cx cy | cy^2           x gp
};

// lane = lane in the wave, (cx, cy) and grad[3] this lane's pixel; *_par are the same quantities of lane ^ 7
__device__ __forceinline__ RowWeights make_row_weights(int lane, float cx, float cy, float g0, float g1, float g2) {
  const bool odd = lane & 4;
  auto partner = [](float v) {
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x141 /* row_half_mirror */, 0xF, 0xF, false));
  };
  RowWeights w;
  w.a_own = odd ? g1 : g0;  w.a_par = partner(odd ? g0 : g1);  // the partner sits in the other kind of bank
  w.b_own = g2;             w.b_par = partner(g2);
  w.c_own = odd ? cx : 1.0f;       w.c_par = partner(odd ? 1.0f : cx);
  w.d_own = odd ? cx * cx : cy;    w.d_par = partner(odd ? cy : cx * cx);
  w.e_own = odd ? cy * cy : cx * cy;  w.e_par = partner(odd ? cx * cy : cy * cy);
  return w;
}

__device__ __forceinline__ float row_moments9(float aT, float gp, const RowWeights &w) {
  float r0, r1, r2, r3, r4;  // few temporaries on purpose: the backward sits at a VGPR-occupancy step
  const unsigned long long odd = 0xAAAAAAAAAAAAAAAAull, bit1 = 0xCCCCCCCCCCCCCCCCull;
  asm volatile(
      // stage A (lane bit 2, partner l ^ 7): the five plain products first, they double as the wait states between
      // the instruction that wrote gp and its first DPP read
      "v_mul_f32 %[r0], %[aT], %[a_own]\n\t"
      "v_mul_f32 %[r1], %[aT], %[b_own]\n\t"
      "v_mul_f32 %[r2], %[gp], %[c_own]\n\t"
      "v_mul_f32 %[r3], %[gp], %[d_own]\n\t"
      "v_mul_f32 %[r4], %[gp], %[e_own]\n\t"
      "v_fmac_f32_dpp %[r0], %[aT], %[a_par] row_half_mirror row_mask:0xf bank_mask:0xf\n\t"
      "v_fmac_f32_dpp %[r1], %[aT], %[b_par] row_half_mirror row_mask:0xf bank_mask:0xf\n\t"
      "v_fmac_f32_dpp %[r2], %[gp], %[c_par] row_half_mirror row_mask:0xf bank_mask:0xf\n\t"
      "v_fmac_f32_dpp %[r3], %[gp], %[d_par] row_half_mirror row_mask:0xf bank_mask:0xf\n\t"
      "v_fmac_f32_dpp %[r4], %[gp], %[e_par] row_half_mirror row_mask:0xf bank_mask:0xf\n\t"
      // stage B: lanes 8 apart (lane bit 3), in place: banks 0,1 keep the even register, banks 2,3 take the odd one
      // (row_shl:8 with bound_ctrl:0 adds 0 in banks 2,3); the (cx cy | cy^2) register pairs with itself: one rotate
      "v_add_f32_dpp %[r0], %[r0], %[r0] row_shl:8 row_mask:0xf bank_mask:0xf bound_ctrl:0\n\t"
      "v_add_f32_dpp %[r0], %[r1], %[r1] row_shr:8 row_mask:0xf bank_mask:0xc bound_ctrl:0\n\t"
      "v_add_f32_dpp %[r2], %[r2], %[r2] row_shl:8 row_mask:0xf bank_mask:0xf bound_ctrl:0\n\t"
      "v_add_f32_dpp %[r2], %[r3], %[r3] row_shr:8 row_mask:0xf bank_mask:0xc bound_ctrl:0\n\t"
      "v_add_f32_dpp %[r4], %[r4], %[r4] row_ror:8 row_mask:0xf bank_mask:0xf\n\t"
      // stage C: lane bit 0: even lanes keep r0, odd lanes r2; r4 is summed in place
      "v_cndmask_b32_e64 %[r1], %[r2], %[r0], %[odd]\n\t"
      "v_cndmask_b32_e64 %[r3], %[r0], %[r2], %[odd]\n\t"
      "s_nop 0\n\t"
      "v_add_f32_dpp %[r4], %[r4], %[r4] quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf\n\t"
      "v_add_f32_dpp %[r1], %[r1], %[r3] quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf\n\t"
      // stage D: lane bit 1: lanes with the bit clear keep r1 (values 0..7), the others the r4 pair
      "v_cndmask_b32_e64 %[r0], %[r4], %[r1], %[bit1]\n\t"
      "v_cndmask_b32_e64 %[r2], %[r1], %[r4], %[bit1]\n\t"
      "s_nop 1\n\t"
      "v_add_f32_dpp %[r0], %[r0], %[r2] quad_perm:[2,3,0,1] row_mask:0xf bank_mask:0xf\n\t"
      : [r0] "=&v"(r0), [r1] "=&v"(r1), [r2] "=&v"(r2), [r3] "=&v"(r3), [r4] "=&v"(r4)
      : [aT] "v"(aT), [gp] "v"(gp), [a_own] "v"(w.a_own), [a_par] "v"(w.a_par), [b_own] "v"(w.b_own),
        [b_par] "v"(w.b_par), [c_own] "v"(w.c_own), [c_par] "v"(w.c_par), [d_own] "v"(w.d_own), [d_par] "v"(w.d_par),
        [e_own] "v"(w.e_own), [e_par] "v"(w.e_par), [odd] "s"(odd), [bit1] "s"(bit1));
  return r0;
}
// which of the nine sums a lane of `out` holds: 0..2 rgb, 3 S_1, 4 S_cx, 5 S_cy, 6 S_cx2, 7 S_cxcy, 8 S_cy2; -1: none
__device__ __host__ __forceinline__ int row_moments9_index(int lane) {
  const int b0 = lane & 1, b1 = (lane >> 1) & 1, b2 = (lane >> 2) & 1, b3 = (lane >> 3) & 1;
  if (b1) return (b0 == 0 && b3 == 0) ? 7 + b2 : -1;  // the (cx cy | cy^2) register: lanes 2 and 6 of the row
  const int a = 4 * b0 + 2 * b3 + b2;                  // A0..A7 = rgb0 rgb1 rgb2 (dup) S_1 S_cx S_cy S_cx2
  return a < 3 ? a : (a == 3 ? -1 : a - 1);
}

// ---- r04: the same nine row sums with the first TWO butterfly stages folded into the products.  A quad = the four
// lanes of one pixel row of the 4x4 block.  Three registers, each the quad-partial of up to four sums (one per lane of
// the quad), built as  F * W_0 + qp1(F) * W_1 + qp2(F) * W_2 + qp3(F) * W_3  (qp_k = the quad permutation lane -> lane ^ k,
// W_k = the weight of the sum THIS lane is responsible for, at the pixel of lane ^ k: loop-invariant lane constants):
//   A from aT: lanes 0..2 of the quad -> rgb0, rgb1, rgb2        (lane 3: weight 0)
//   B from gp: lanes 0..3             -> S_1, S_cx, S_cy, S_cx2
//   C from gp: lanes 0..1             -> S_cxcy, S_cy2           (lanes 2, 3: weight 0)
// = 3 v_mul + 9 v_fmac_dpp; then the four quads (= DPP banks) of the row are summed with the masked-bank pairs of
// row_sum9: lanes 4 apart fold A and B into one register (banks 0,2: A, banks 1,3: B; 2 instructions) and C onto itself (1),
// lanes 8 apart fold that pair (banks 0,1: the A / B totals; banks 2,3: C's; 2 instructions).  17 VALU + one wait state
// instead of 22 + three; bank 0 ends with the rgb totals, bank 1 with S_1 S_cx S_cy S_cx2, lanes 8, 9 with S_cxcy S_cy2.
struct QuadWeights { float a[4], b[4], c[4]; };

// lane = lane in the wave, (cx, cy) and grad[3] this lane's pixel (cx relative to the tile centre: the lanes of a quad are
// four pixels in a row, lane ^ k sits (lane ^ k) - lane pixels to the right)
__device__ __forceinline__ QuadWeights make_quad_weights(int lane, float cx, float cy, float g0, float g1, float g2) {
  const int p = lane & 3;
  QuadWeights w;
  auto qp = [](float v, auto ctrl) {
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), decltype(ctrl)::value, 0xF, 0xF, false));
  };
  // rgb: the lane that will RECEIVE through qp_k is lane ^ k, responsible for channel p ^ k: this lane offers that channel
  auto offer = [&](int k) { const int ch = p ^ k; return ch == 0 ? g0 : ch == 1 ? g1 : ch == 2 ? g2 : 0.0f; };
  w.a[0] = offer(0);
  w.a[1] = qp(offer(1), std::integral_constant<int, 0xB1>{});  // quad_perm [1,0,3,2]
  w.a[2] = qp(offer(2), std::integral_constant<int, 0x4E>{});  // quad_perm [2,3,0,1]
  w.a[3] = qp(offer(3), std::integral_constant<int, 0x1B>{});  // quad_perm [3,2,1,0]
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const float cxk = cx + (float)((p ^ k) - p);  // pixel of lane ^ k (same row: cy is shared)
    w.b[k] = p == 0 ? 1.0f : p == 1 ? cxk : p == 2 ? cy : cxk * cxk;
    w.c[k] = p == 0 ? cxk * cy : p == 1 ? cy * cy : 0.0f;
  }
  return w;
}

__device__ __forceinline__ float row_moments9q(float aT, float gp, const QuadWeights &w) {
  float A, B, C;
  asm volatile(
      // the three plain products first: they are also the wait states between the instruction that wrote gp and its
      // first DPP read
      "v_mul_f32 %[A], %[aT], %[a0]\n\t"
      "v_mul_f32 %[B], %[gp], %[b0]\n\t"
      "v_mul_f32 %[C], %[gp], %[c0]\n\t"
      "v_fmac_f32_dpp %[C], %[gp], %[c1] quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf\n\t"
      "v_fmac_f32_dpp %[C], %[gp], %[c2] quad_perm:[2,3,0,1] row_mask:0xf bank_mask:0xf\n\t"
      "v_fmac_f32_dpp %[C], %[gp], %[c3] quad_perm:[3,2,1,0] row_mask:0xf bank_mask:0xf\n\t"
      "v_fmac_f32_dpp %[A], %[aT], %[a1] quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf\n\t"
      "v_fmac_f32_dpp %[A], %[aT], %[a2] quad_perm:[2,3,0,1] row_mask:0xf bank_mask:0xf\n\t"
      "v_fmac_f32_dpp %[A], %[aT], %[a3] quad_perm:[3,2,1,0] row_mask:0xf bank_mask:0xf\n\t"
      "v_fmac_f32_dpp %[B], %[gp], %[b1] quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf\n\t"
      "v_fmac_f32_dpp %[B], %[gp], %[b2] quad_perm:[2,3,0,1] row_mask:0xf bank_mask:0xf\n\t"
      "v_fmac_f32_dpp %[B], %[gp], %[b3] quad_perm:[3,2,1,0] row_mask:0xf bank_mask:0xf\n\t"
      // quads 4 lanes apart: C onto itself (banks 0 and 2 end with the pair sums), then A | B into A (banks 0,2 | 1,3)
      "v_add_f32_dpp %[A], %[A], %[A] row_shl:4 row_mask:0xf bank_mask:0xf bound_ctrl:0\n\t"
      "v_add_f32_dpp %[A], %[B], %[B] row_shr:4 row_mask:0xf bank_mask:0xa bound_ctrl:0\n\t"
      "v_add_f32_dpp %[C], %[C], %[C] row_shl:4 row_mask:0xf bank_mask:0xf bound_ctrl:0\n\t"
      // quads 8 lanes apart: banks 0,1 keep the A | B totals, banks 2,3 take C's (bank 2: the total, bank 3: unused).
      // (a VGPR written by VALU may be read through DPP two wait states later: C's fold and the s_nop cover A)
      "s_nop 0\n\t"
      "v_add_f32_dpp %[A], %[A], %[A] row_shl:8 row_mask:0xf bank_mask:0xf bound_ctrl:0\n\t"
      "v_add_f32_dpp %[A], %[C], %[C] row_shr:8 row_mask:0xf bank_mask:0xc bound_ctrl:0\n\t"
      : [A] "=&v"(A), [B] "=&v"(B), [C] "=&v"(C)
      : [aT] "v"(aT), [gp] "v"(gp), [a0] "v"(w.a[0]), [a1] "v"(w.a[1]), [a2] "v"(w.a[2]), [a3] "v"(w.a[3]),
        [b0] "v"(w.b[0]), [b1] "v"(w.b[1]), [b2] "v"(w.b[2]), [b3] "v"(w.b[3]), [c0] "v"(w.c[0]), [c1] "v"(w.c[1]),
        [c2] "v"(w.c[2]), [c3] "v"(w.c[3]));
  return A;
}
// which of the nine sums a lane holds after row_moments9q (0..2 rgb, 3 S_1, 4 S_cx, 5 S_cy, 6 S_cx2, 7 S_cxcy, 8 S_cy2; -1: none)
__device__ __host__ __forceinline__ int row_moments9q_index(int lane) {
  const int j = lane & 15;
  return j < 3 ? j : (j >= 4 && j < 8) ? j - 1 : j == 8 ? 7 : j == 9 ? 8 : -1;
}

// ---- r04 (second half): the same nine row sums in 14 VALU.  The four lanes of a quad are four pixels of ONE pixel row,
// so inside a quad cy is a constant: the quad-partials of S_cy, S_cxcy and S_cy2 are cy x S_1, cy x S_cx and cy^2 x S_1 of
// the same quad.  The quad stage therefore builds only two registers,
//   A from aT: lanes 0..2 of the quad -> rgb0, rgb1, rgb2           (lane 3: weight 0)
//   B from gp: lanes 0..3             -> S_1, S_cx, S_cx2, S_1 (again)
// (2 v_mul + 6 v_fmac_dpp), one more product forms  Q = B x (cy, cy, 0, cy^2)  = the quad-partials of S_cy, S_cxcy, -,
// S_cy2, and the four quads of the row are summed as in row_moments9q (A | B into banks 0,2 | 1,3, Q onto itself, then
// the halves: 5 masked DPP adds).  Bank 0 ends with the rgb totals, bank 1 with S_1 S_cx S_cx2 (S_1), bank 2 with S_cy
// S_cxcy - S_cy2.  The wait state the last fold needs is filled by the caller's own instruction: the LDS address of the
// atomic that follows (addr = off * 5 + acc_lane), which the loop needs anyway.
struct RowsWeights { float a[4], b[4], q; };

// kFourth: the quad's fourth lane weighs aT with g3 instead of 0 -- depth mode (DepthMaps, below) passes dL/d depth, and
// lane 3 of the row ends with a tenth total, sum aT x dL/d depth, at no extra instruction in the loop.  (A template, not
// a defaulted argument: with g3 = 0 as an argument the default kernels' register allocation changed, 2 -> 19 spills.)
template <bool kFourth = false>
__device__ __forceinline__ RowsWeights make_rows_weights(int lane, float cx, float cy, float g0, float g1, float g2,
                                                         float g3 = 0.0f) {
  const int p = lane & 3;
  RowsWeights w;
  auto qp = [](float v, auto ctrl) {
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), decltype(ctrl)::value, 0xF, 0xF, false));
  };
  auto offer = [&](int k) {
    const int ch = p ^ k;
    if constexpr (kFourth) return ch == 0 ? g0 : ch == 1 ? g1 : ch == 2 ? g2 : g3;
    else return ch == 0 ? g0 : ch == 1 ? g1 : ch == 2 ? g2 : 0.0f;
  };
  w.a[0] = offer(0);
  w.a[1] = qp(offer(1), std::integral_constant<int, 0xB1>{});  // quad_perm [1,0,3,2]
  w.a[2] = qp(offer(2), std::integral_constant<int, 0x4E>{});  // quad_perm [2,3,0,1]
  w.a[3] = qp(offer(3), std::integral_constant<int, 0x1B>{});  // quad_perm [3,2,1,0]
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const float cxk = cx + (float)((p ^ k) - p);  // pixel of lane ^ k (same pixel row)
    w.b[k] = p == 1 ? cxk : p == 2 ? cxk * cxk : 1.0f;
  }
  w.q = p == 3 ? cy * cy : p == 2 ? 0.0f : cy;
  return w;
}

// returns the register of the totals; `addr` <- off * kMul + acc_lane (the caller's atomic address, computed in the wait
// state; kMul = 5: ten doubles per slot, 6: the moment option's twelve, gs_render.h: DepthMaps)
template <int kMul = 5>
__device__ __forceinline__ float row_moments9r(float aT, float gp, const RowsWeights &w, unsigned int off, unsigned int acc_lane,
                                               unsigned int &addr) {
  float A, B, Q;
  asm volatile(
      // the two plain products first: the wait states between the instructions that wrote aT / gp and their first DPP read
      "v_mul_f32 %[A], %[aT], %[a0]\n\t"
      "v_mul_f32 %[B], %[gp], %[b0]\n\t"
      "v_fmac_f32_dpp %[A], %[aT], %[a1] quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf\n\t"
      "v_fmac_f32_dpp %[B], %[gp], %[b1] quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf\n\t"
      "v_fmac_f32_dpp %[A], %[aT], %[a2] quad_perm:[2,3,0,1] row_mask:0xf bank_mask:0xf\n\t"
      "v_fmac_f32_dpp %[B], %[gp], %[b2] quad_perm:[2,3,0,1] row_mask:0xf bank_mask:0xf\n\t"
      "v_fmac_f32_dpp %[A], %[aT], %[a3] quad_perm:[3,2,1,0] row_mask:0xf bank_mask:0xf\n\t"
      "v_fmac_f32_dpp %[B], %[gp], %[b3] quad_perm:[3,2,1,0] row_mask:0xf bank_mask:0xf\n\t"
      "v_mul_f32 %[Q], %[B], %[wq]\n\t"
      // quads 4 lanes apart: A | B into A (banks 0,2 | 1,3), Q onto itself (banks 0 and 2 end with the pair sums)
      "v_add_f32_dpp %[A], %[A], %[A] row_shl:4 row_mask:0xf bank_mask:0xf bound_ctrl:0\n\t"
      "v_add_f32_dpp %[A], %[B], %[B] row_shr:4 row_mask:0xf bank_mask:0xa bound_ctrl:0\n\t"
      "v_add_f32_dpp %[Q], %[Q], %[Q] row_shl:4 row_mask:0xf bank_mask:0xf bound_ctrl:0\n\t"
      // (a VGPR written by VALU may be read through DPP two wait states later: Q's fold and the address cover A)
      "v_mad_u32_u24 %[addr], %[off], %[mul], %[acc]\n\t"
      // quads 8 lanes apart: banks 0,1 keep the A | B totals, banks 2,3 take Q's (bank 2: the total, bank 3: unused)
      "v_add_f32_dpp %[A], %[A], %[A] row_shl:8 row_mask:0xf bank_mask:0xf bound_ctrl:0\n\t"
      "v_add_f32_dpp %[A], %[Q], %[Q] row_shr:8 row_mask:0xf bank_mask:0xc bound_ctrl:0\n\t"
      : [A] "=&v"(A), [B] "=&v"(B), [Q] "=&v"(Q), [addr] "=&v"(addr)
      : [aT] "v"(aT), [gp] "v"(gp), [a0] "v"(w.a[0]), [a1] "v"(w.a[1]), [a2] "v"(w.a[2]), [a3] "v"(w.a[3]),
        [b0] "v"(w.b[0]), [b1] "v"(w.b[1]), [b2] "v"(w.b[2]), [b3] "v"(w.b[3]), [wq] "v"(w.q), [off] "v"(off),
        [acc] "v"(acc_lane), [mul] "n"(kMul));
  return A;
}
// which of the nine sums a lane holds after row_moments9r (0..2 rgb, 3 S_1, 4 S_cx, 5 S_cy, 6 S_cx2, 7 S_cxcy, 8 S_cy2; -1: none)
__device__ __host__ __forceinline__ int row_moments9r_index(int lane) {
  const int j = lane & 15;
  return j < 3 ? j : j == 4 ? 3 : j == 5 ? 4 : j == 6 ? 6 : j == 8 ? 5 : j == 9 ? 7 : j == 11 ? 8 : -1;
}

// row_moments9r without the colour sums (features_bwd_kernel: the colours are the caller's): the six moments of gp only,
// in the lanes row_moments9r_index gives them (sums 3..8).  The same instructions with the same spacing; the register of
// the colour totals starts as zero instead of the four aT products, which frees the four colour weights and aT itself
// (lanes 0..2 of the result hold zeros and are not added).  `addr` <- off * kMul + acc_lane as there.
template <int kMul>
__device__ __forceinline__ float row_moments6r(float gp, const RowsWeights &w, unsigned int off, unsigned int acc_lane,
                                               unsigned int &addr) {
  float A, B, Q;
  asm volatile(
      // two plain instructions first: the wait states between the instruction that wrote gp and its first DPP read
      "v_mul_f32 %[B], %[gp], %[b0]\n\t"
      "v_mov_b32 %[A], 0\n\t"
      "v_fmac_f32_dpp %[B], %[gp], %[b1] quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf\n\t"
      "v_fmac_f32_dpp %[B], %[gp], %[b2] quad_perm:[2,3,0,1] row_mask:0xf bank_mask:0xf\n\t"
      "v_fmac_f32_dpp %[B], %[gp], %[b3] quad_perm:[3,2,1,0] row_mask:0xf bank_mask:0xf\n\t"
      "v_mul_f32 %[Q], %[B], %[wq]\n\t"
      "v_add_f32_dpp %[A], %[A], %[A] row_shl:4 row_mask:0xf bank_mask:0xf bound_ctrl:0\n\t"
      "v_add_f32_dpp %[A], %[B], %[B] row_shr:4 row_mask:0xf bank_mask:0xa bound_ctrl:0\n\t"
      "v_add_f32_dpp %[Q], %[Q], %[Q] row_shl:4 row_mask:0xf bank_mask:0xf bound_ctrl:0\n\t"
      "v_mad_u32_u24 %[addr], %[off], %[mul], %[acc]\n\t"
      "v_add_f32_dpp %[A], %[A], %[A] row_shl:8 row_mask:0xf bank_mask:0xf bound_ctrl:0\n\t"
      "v_add_f32_dpp %[A], %[Q], %[Q] row_shr:8 row_mask:0xf bank_mask:0xc bound_ctrl:0\n\t"
      : [A] "=&v"(A), [B] "=&v"(B), [Q] "=&v"(Q), [addr] "=&v"(addr)
      : [gp] "v"(gp), [b0] "v"(w.b[0]), [b1] "v"(w.b[1]), [b2] "v"(w.b[2]), [b3] "v"(w.b[3]), [wq] "v"(w.q), [off] "v"(off),
        [acc] "v"(acc_lane), [mul] "n"(kMul));
  return A;
}

// ---- absgrad mode (gsplat_context_set_absgrad): the same sums plus the row totals of two per-pixel ABSOLUTE values,
//   U = |gp| |pu|,  V = |gp| |pv|,   (pu, pv) = (2 a2 dx + b2 dy, 2 c2 dy + b2 dx)  in the staged conic (stage_record),
// i.e. |d/du| and |d/dv| of this pixel's share up to the per-gaussian factor -kConicOff x (0.5 W | 0.5 H) the flush
// applies.  They cannot ride in the quad stage's v_fmac_dpp (neither factor is a lane constant), so they take the
// masked-bank route of row_sum9: lanes 4 apart fold U | V into one register (banks 0,2 | 1,3: 2 instructions), lanes 8
// apart one rotate, then the two quad steps -- 2 products + 5 DPP adds.  Bank 2 ends with U's total in every lane, bank 3
// with V's; one v_cndmask parks them in the two lanes of the totals' register that carry nothing (lane 10: Q's zero
// weight, lane 12: bank 3), so the ONE LDS atomic of the trip adds them too.  10 VALU on top of row_moments9r's 14, no
// s_nop: every DPP read of U sits two instructions behind its write, with the colour / moment chain's instructions in
// between; that chain is row_moments9r's, operation for operation (the nine sums are bit for bit those of the mode off).
// The accumulators are twelve doubles per slot here: addr <- off * 6 + acc_lane.
__device__ __forceinline__ float row_moments9r_abs(float aT, float gp, float pu, float pv, const RowsWeights &w, unsigned int off,
                                                   unsigned int acc_lane, unsigned int &addr) {
  float A, B, Q, U, V;
  const unsigned long long park = 0x1400140014001400ull;  // lanes 10 and 12 of every row
  asm volatile(
      "v_mul_f32_e64 %[U], |%[gp]|, |%[pu]|\n\t"
      "v_mul_f32_e64 %[V], |%[gp]|, |%[pv]|\n\t"
      "v_mul_f32 %[A], %[aT], %[a0]\n\t"
      "v_mul_f32 %[B], %[gp], %[b0]\n\t"
      "v_fmac_f32_dpp %[A], %[aT], %[a1] quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf\n\t"
      "v_fmac_f32_dpp %[B], %[gp], %[b1] quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf\n\t"
      "v_add_f32_dpp %[U], %[U], %[U] row_shl:4 row_mask:0xf bank_mask:0xf bound_ctrl:0\n\t"
      "v_add_f32_dpp %[U], %[V], %[V] row_shr:4 row_mask:0xf bank_mask:0xa bound_ctrl:0\n\t"
      "v_fmac_f32_dpp %[A], %[aT], %[a2] quad_perm:[2,3,0,1] row_mask:0xf bank_mask:0xf\n\t"
      "v_fmac_f32_dpp %[B], %[gp], %[b2] quad_perm:[2,3,0,1] row_mask:0xf bank_mask:0xf\n\t"
      "v_add_f32_dpp %[U], %[U], %[U] row_ror:8 row_mask:0xf bank_mask:0xf\n\t"
      "v_fmac_f32_dpp %[A], %[aT], %[a3] quad_perm:[3,2,1,0] row_mask:0xf bank_mask:0xf\n\t"
      "v_fmac_f32_dpp %[B], %[gp], %[b3] quad_perm:[3,2,1,0] row_mask:0xf bank_mask:0xf\n\t"
      "v_add_f32_dpp %[U], %[U], %[U] quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf\n\t"
      "v_mul_f32 %[Q], %[B], %[wq]\n\t"
      "v_add_f32_dpp %[A], %[A], %[A] row_shl:4 row_mask:0xf bank_mask:0xf bound_ctrl:0\n\t"
      "v_add_f32_dpp %[U], %[U], %[U] quad_perm:[2,3,0,1] row_mask:0xf bank_mask:0xf\n\t"
      "v_add_f32_dpp %[A], %[B], %[B] row_shr:4 row_mask:0xf bank_mask:0xa bound_ctrl:0\n\t"
      "v_add_f32_dpp %[Q], %[Q], %[Q] row_shl:4 row_mask:0xf bank_mask:0xf bound_ctrl:0\n\t"
      "v_mad_u32_u24 %[addr], %[off], 6, %[acc]\n\t"
      "v_add_f32_dpp %[A], %[A], %[A] row_shl:8 row_mask:0xf bank_mask:0xf bound_ctrl:0\n\t"
      "v_add_f32_dpp %[A], %[Q], %[Q] row_shr:8 row_mask:0xf bank_mask:0xc bound_ctrl:0\n\t"
      "v_cndmask_b32_e64 %[A], %[A], %[U], %[park]\n\t"
      : [A] "=&v"(A), [B] "=&v"(B), [Q] "=&v"(Q), [U] "=&v"(U), [V] "=&v"(V), [addr] "=&v"(addr)
      : [aT] "v"(aT), [gp] "v"(gp), [pu] "v"(pu), [pv] "v"(pv), [a0] "v"(w.a[0]), [a1] "v"(w.a[1]), [a2] "v"(w.a[2]),
        [a3] "v"(w.a[3]), [b0] "v"(w.b[0]), [b1] "v"(w.b[1]), [b2] "v"(w.b[2]), [b3] "v"(w.b[3]), [wq] "v"(w.q),
        [off] "v"(off), [acc] "v"(acc_lane), [park] "s"(park));
  return A;
}
// row_moments9r_index plus the two parked totals: 10 = sum |gp pu|, 11 = sum |gp pv|
__device__ __host__ __forceinline__ int row_moments9r_abs_index(int lane) {
  const int j = lane & 15;
  return j == 10 ? 10 : j == 12 ? 11 : row_moments9r_index(lane);
}

// Blocks are dealt round-robin over the 8 XCDs; give each XCD a contiguous run of tiles so
// neighbouring tiles (which share gaussians) hit the same L2.  Returns >= num_tiles for the
// padding blocks of the last round.
__device__ __forceinline__ int block_to_tile(int block, int num_tiles) {
  const int per_xcd = (num_tiles + 7) >> 3;
  return (block & 7) * per_xcd + (block >> 3);
}
static inline int tile_grid(int num_tiles) { return ((num_tiles + 7) >> 3) * 8; }
// r04: the same map through an optional order table (tile_order_kernel, gs_render_bwd.hip): slot s of the table holds the tile
// that the block mapped to slot s should take -- every XCD's run of tiles re-ordered heaviest first, so that the
// launch's last round is made of its lightest tiles (entries >= num_tiles: padding)
__device__ __forceinline__ int ordered_tile(const int *__restrict__ order, int block, int num_tiles) {
  const int slot = block_to_tile(block, num_tiles);
  return order ? order[slot] : slot;
}
constexpr int kOrderMaxRun = 2048;  // tiles per XCD run the order kernel handles (16384 tiles: the counting-sort limit)
constexpr int kTableChunks = 16;    // tiles per thread of the one-workgroup segment tables (tile_segments_kernel, fwd_segments_table_kernel)

// r05 -- long tile lists, split for the BACKWARD.  One workgroup walks one tile's list batch after batch: a list of ten
// thousand entries is eighty batches in a row, and on a trained capture (lists of 1100 entries on average, 9800 at most)
// that ONE chain was the duration of the whole launch -- render_bwd 0.72 ms with the VALU 19 % busy.  The back-to-front
// recurrence only needs, at a boundary b of the list, the transmittance in front of entry b and the colour composited
// behind it; the forward passes both through anyway.  So for tiles whose list exceeds kSegSplitMin entries the forward
// stores, at every kSegEntries-th entry it reaches, a per-pixel checkpoint {T_b, C_b} (C_b: the colour accumulated from
// the entries in front of b, without the background), and the backward gives every segment [k kSegEntries,
// (k+1) kSegEntries) that some pixel of the tile reaches a workgroup of its own: a pixel that stops behind the segment
// starts it from T_b and the colour (image - C_b) / T_b behind it, a pixel that stops inside or in front of it from its
// final transmittance as before.  The gradient rows are added with atomics either way.
//   Checkpoint slots need no table: the boundary k >= 1 of the tile whose list starts at instance r has the slot
// r / kSegEntries + k (boundaries are kSegEntries instances apart inside a list and further apart across lists, so no two
// share a slot; the pool has room / kSegEntries + 2 slots).  Which segments exist is decided BEHIND the forward, from the
// tiles' largest stop indices (tile_segments_kernel): segment 0 of every tile is the block the tile has always had, the
// further segments are extra blocks in front of the main grid, listed in `extra`; granted[t] = how many tile t got
// (0: its block walks the whole list, also when the launch's room for extra blocks was used up).
#ifndef GS_SEG_ENTRIES
#define GS_SEG_ENTRIES 496
#endif
constexpr int kSegEntries = GS_SEG_ENTRIES;  // 2 forward batches = 4 backward batches
#ifndef GS_SEG_SPLIT_MIN
#define GS_SEG_SPLIT_MIN (3 * GS_SEG_ENTRIES)
#endif
constexpr int kSegSplitMin = GS_SEG_SPLIT_MIN;  // lists up to here stay whole
struct TileSegments {
  int *granted;            // [num_tiles]: further segments of the tile in `extra` (written behind the forward)
  int2 *extra;             // [extra_cap]: (tile, k) of the segments k >= 1
  int *extra_count;        // [1]
  float4 *chk;             // [slots][256]: one checkpoint per boundary, per pixel of the tile (thread order)
  const float *image;      // the forward's image (the backward's view of the colour behind a boundary)
  int extra_cap;           // room in `extra`; a multiple of 8 (the main blocks keep their XCDs)
  // Host-visible figures of this forward, each ONE 8-byte word {the forward's ticket << 32 | value} (gs_common.h: the
  // record's form), in the slot of the ticket's parity: the host takes a slot only when it carries the ticket of a forward
  // whose kernels it knows to have completed (r06, ADVICE r05: the plain ints of r05 were read while the kernels that
  // write them could still be running, and the forward's split decision followed host / GPU timing).
  unsigned long long *asked;  // [1]: the segments the tiles asked for (sizes a later launch's room)
  unsigned long long *stats;  // [2]: the largest stop index of any tile | the sum of the tiles' largest stop indices
  unsigned int tag;           // low half of the forward's ticket
};
__host__ __device__ inline unsigned long long tagged_figure(unsigned int tag, int value) {
  return ((unsigned long long)tag << 32) | (unsigned int)value;
}
__host__ __device__ inline int segment_slot(int list_start, int boundary) { return list_start / kSegEntries + boundary; }

// r05 -- the same long lists in the FORWARD.  The front-to-back recurrence is serial in the transmittance only: a
// segment k of a list can composite on its own once it knows P_k, the T in front of its first entry.  Every segment of a
// long list is a block of its own (fwd_segment_block), and the blocks are dispatched LAYER by layer: all segments 0,
// then all segments 1, ...
//  * Where a layer fills the chip, the layer behind it starts when it is through: a block finds the final T of the block
//    in front of it (F_(k-1) = P_k) already published, composites (phase C), and publishes its own.  A segment no pixel
//    reaches finds only zeros and leaves at once.  This is the unsplit forward's work, dealt in equal pieces.
//  * In the thin layers of the few longest lists the blocks run side by side.  A block that does not find F_(k-1) first
//    multiplies up the transmittance t_k of ITS entries per pixel (phase A: alpha evaluation only, no colour, no stop
//    logic: ~70 % of a compositing pass) and publishes it, then collects P_k = F_q t_(q+1) ... t_(k-1) from the nearest
//    finished block q in front of it and the products behind that, and composites.
// Published values are 8-byte {launch epoch, value} granules per pixel, written and polled with agent-scope atomics: the
// data is its own flag.  Phase C runs with T = P_k * t, t the running product inside the segment -- bit for bit the
// sequence phase A multiplied up -- so F_k = P_k t_k = P_(k+1) exactly, whichever way a block obtained it: a pixel that
// has not stopped in segment k (every T >= 1e-4) is live in segment k + 1, one that has stopped (T < 1e-4 at some entry)
// is dead there, whatever the rounding -- no pixel is lost or composited twice.  Segment 0 (P = 1) is the unsplit
// arithmetic.  A block only ever waits for blocks with smaller indices (workgroups are dispatched in index order) and
// not for ever: when its poll budget is used up it multiplies the product up itself from entry 0 (same values), so
// every wave reaches its end whatever the dispatch order.  A one-block-per-tile kernel behind the forward
// (fwd_segments_combine_kernel) adds the segments' colours in order, finds the segment in which the pixel stopped and
// writes image / T / stop index / the backward's checkpoints: sums in a fixed order, the same image in every run.
struct FwdSegments {
  int *rank;                     // [num_tiles]: the tile's rank among the long lists (most segments first), -1: one block
  int *base;                     // [129]: first block of layer k; segment (t, k) is block (= storage slot) base[k] + rank[t]
  int2 *blocks;                  // [cap]: (tile, k | thin-layer flag << 30) by block
  int *count;                    // [1]: blocks in use
  unsigned long long *granules;  // [2][cap][256]: {epoch, value} per block and pixel: t_k | the T behind segment k
  float4 *part;                  // [cap][256]: the segment's colour and the T behind it (its final T if the pixel stopped)
  int *stop;                     // [cap][256]: the stop index if the pixel stopped in the segment, -1 live, -2 dead
  int cap;                       // room for segment blocks; a multiple of 8 (the main blocks keep their XCDs)
  unsigned int epoch;            // of this launch; never 0
  unsigned long long *asked;     // [1], host-visible, {ticket << 32 | value} (see TileSegments): segment blocks the lists asked for
  unsigned int tag;              // low half of the forward's ticket
  int *fallbacks;                // [1], device: segment blocks whose polls ran out and which multiplied the product up themselves
  int poll_budget;               // polls (~1 us each) before a segment block multiplies the product up itself
  int thin_layer;                // layers of fewer blocks run their lists' segments side by side (phase A)
};
// r06: 128 polls ~ 0.13 ms, a dozen segments' worth of compositing -- a block whose predecessor is not even
// resident (the dispatch order it relies on is an assumption) recomputes after that instead of after 4 ms (r05: 4096),
// and every such block is counted (gsplat_context_get_counters out[9]).
constexpr int kFwdPollBudget = 128, kFwdThinLayerDefault = 512;  // (gsplat_context_set_segment_options changes them)

// Depth mode (gsplat_context_set_depth): the packed compositing kernels' <.., kDepth = true> instantiations carry one more
// "colour channel", the camera-space depth z of every gaussian, composited over a background of 0:
//   depth(p) = sum_{i < n(p)} alpha_i T_i z_i        (alpha(p) = 1 - T(p) needs nothing of its own)
// The forward stages z in the slot of the LDS record its loop does not read (r1.z, the plain opacity), the backward in
// r1.w (the footprint's hy); the global 48-byte record is unchanged.  The long-list machinery gets side arrays at the
// slots of the colour ones: a segment's partial depth next to FwdSegments::part, the depth so far next to
// TileSegments::chk.  The backward takes dL/d depth and dL/d alpha per pixel and adds sum aT * dL/d depth (= dL/d z) as
// the tenth value of the gaussian's gradient row (slot 9), which preprocess_bwd_kernel adds to dL/d z_c.
//
// Two options of the mode (gsplat_context_set_depth_mode), each a template parameter of the kernels: the instantiations
// with both off are the ones above, untouched.
//  * inverse: the composited value is s = 1/z instead of z.  Staging writes s into the record's slot (r1.z forward, r1.w
//    backward, the segment paths included) as ONE v_rcp_f32 (depth_value: 1 ulp, not an IEEE division -- both directions
//    use the same instruction, so the backward sees the forward's s bit for bit; z > near_thresh > 0 for every compacted
//    gaussian, so s is finite).  The chain rule ds/dz = -s^2 is applied where slot 9 is formed, in the backward's flush
//    step 1: slot 9 stays dL/dz_c and preprocess_bwd_kernel is the depth mode's.
//  * moment: the forward also composites Q(p) = sum_{i < n(p)} alpha_i T_i s_i^2 over background 0 (one multiply and one FMA
//    next to the depth's), with side arrays next to the depth's (part2, chk2), and the backward takes a third map
//    G_Q = dL/dQ: t gains s^2 G_Q (the depth's FMA becomes s (G_D + s G_Q), two), a segment entered at a boundary starts
//    from (Q image - Q so far) / T_b as well, and dL/ds_i = sum_p aT G_D + 2 s_i sum_p aT G_Q needs one more row total.
//    Route of that total: aT G_Q is no lane constant times aT once the colour register's four quad lanes are taken
//    (rgb and G_D), so it is summed over the row on its own -- one product and the four DPP adds of row_sum -- and parked
//    in lane 10 of the totals' register (Q's zero weight, as absgrad parks its first), where the trip's single
//    ds_add_f64 adds it to accumulator 10; the accumulators are twelve doubles per slot as in absgrad mode
//    (row_moments9r<6>).  The flush forms  res[9] = keep (acc[9] + 2 s acc[10]) (inverse ? -s^2 : 1)  in double.
//    moment together with absgrad is REFUSED (GSPLAT_ERR_INVALID_ARG before anything is launched): absgrad parks its two
//    totals in lanes 10 and 12 and fills accumulators 10 and 11, and a fourteen-double slot does not fit the kernel's LDS
//    at seven workgroups per CU.
struct DepthMaps {
  const float *xyz_c;       // [M,3] compacted camera-space positions (the context's c->xyz_c)
  float *depth;             // [H,W] the forward writes it; the backward reads it at segment boundaries
  float *part;              // [FwdSegments::cap][256] a segment's partial depth (its own entries only)
  float *chk;               // [TileSegments slots][256] the depth accumulated in front of a boundary
  const float *grad_depth;  // [H,W] backward: dL/d depth (null: zero)
  const float *grad_alpha;  // [H,W] backward: dL/d alpha (null: zero)
  // the options (both off: everything below is unused)
  float *depth2;             // [H,W] moment: Q, written and read like `depth`
  float *part2;              // moment: a segment's partial Q, beside `part`
  float *chk2;               // moment: Q so far, beside `chk`
  const float *grad_depth2;  // [H,W] backward, moment: dL/dQ (null: zero)
  bool inverse, moment;      // which instantiation the launchers pick
};

// what depth mode composites for a gaussian at camera-space depth z
template <bool kInv>
__device__ __forceinline__ float depth_value(float z) {
  if constexpr (kInv) return __builtin_amdgcn_rcpf(z);
  else return z;
}

// Compact lists for the backward (gsplat_context_set_compact_lists).  The tile lists come from the reference's box test,
// and about a quarter of their entries (benchmark scene: 23.7 %) reach no 4x4 block of their tile with alpha >= 1/255:
// block_hits gives them an empty mask, they enter no row list, and they add nothing to the image or to any gradient.  The
// backward still staged them, gave them a slot of its batches and flushed their zeros.  The forward, which computes every
// entry's mask anyway, therefore writes each tile's USEFUL entries (mask != 0), in list order, to the front of the tile's
// own range of `ids` / `masks`, and per pixel the stop index counted in useful entries: render_bwd_kernel given these three
// arrays in place of sorted / masks / n walks only the useful entries, with the same per-pixel arithmetic.  The full lists,
// masks and stop indices are written as ever (parity outputs; contributions_kernel reads them).
struct CompactLists {
  int *ids;               // [instances]: per tile, the useful entries of its list, a prefix of [ranges[t], ranges[t + 1])
  unsigned short *masks;  // [instances]: their block masks, same positions
  int *n_px;              // [H,W]: useful entries in front of and including the one that saturated the pixel
  int *count;             // [num_tiles]: useful entries the tile's workgroup ranked (all of them unless every pixel saturated)
};

struct RawSplats {  // the reference operator's input arrays
  const float *uv, *opacity, *conic, *rgb;
};
struct GradOut {         // either whole rows ...
  float *rows;           // [M,16]: rgb3 opacity1 conic3 uv2, 7 pad
  // ... or the reference operator's four arrays
  float *rgb, *opacity, *uv, *conic;
};

// ---- What the two compositing launchers take (gs_launch.h).  A caller starts from {} and assigns members by name; whatever
// it leaves alone is off.  The option structs are held by value and a value-initialised one means "off", which is how the
// kernels read them: TileSegments is on when chk is set, FwdSegments when blocks is, CompactLists when ids is, and
// DepthMaps -- depth mode -- when xyz_c is.  The gaussians come as `recs` (the context's packed 48-byte records) or as
// `raw` (the reference operator's arrays), never both.
struct RenderFwdArgs {
  const float4 *recs;
  RawSplats raw;
  const int *sorted, *ranges;  // the tile lists
  int width, height;
  float bg;
  int *n_out;    // [H,W] per pixel: the stop index ...
  float *T_out;  // ... the final transmittance ...
  float *image;  // ... and the colour
  float4 *zero;        // optional: `zero_vec` float4 the kernel clears on the side (the backward's gradient rows)
  long long zero_vec;
  unsigned short *masks_out;  // optional, per instance: the block masks, for the backward
  int *tops_out;              // optional, per tile: the largest stop index of its pixels
  TileSegments segments;      // the backward's checkpoints of long lists
  FwdSegments fwd_segments;   // long lists as blocks of their own
  DepthMaps depth;
  CompactLists compact;       // the context's unsegmented forward only
};
struct RenderBwdArgs {
  const float4 *recs;
  RawSplats raw;
  const int *sorted, *ranges;  // the tile lists (compact lists: their useful entries, with `masks_in` and `n_px` to match)
  const int *n_px;             // [H,W] the forward's stop indices ...
  const float *T_px;           // ... and final transmittances
  const float *grad_image;
  int width, height;
  float bg;
  GradOut out;                     // rows, or the four arrays
  const unsigned short *masks_in;  // the forward's block masks (packed records only; the raw form computes them)
  const int *order;                // optional: the tiles heaviest first (launch_tile_order)
  hipEvent_t ev_start, ev_stop;    // optional, both or neither: the launch stamps them itself
  TileSegments segments;
  DepthMaps depth;  // depth mode: needs recs and out.rows
  bool absgrad;     // likewise
};
// A recorded forward, as the kernels that walk it again take it (gs_replay.hip): the context's packed records, the full
// tile lists and the forward's per-pixel outputs.
struct ReplayArgs {
  const float4 *recs;
  const int *sorted, *ranges;  // the tile lists
  const int *n_px;             // [H,W] the forward's stop indices ...
  const float *T_px;           // ... and final transmittances (read by features_bwd_kernel only)
  const int *c2g;              // compact_to_global
  int width, height;
};

// ---- what the compositing and the replay kernels share of the tile walk -----------------------------------------------
// Diagnostic build (-DGS_STAMP=1, tools/bwd_timeline.py): every wave of render_fwd / render_bwd records where its cycles
// went (s_memtime around the barriers, staging, list building, the trip loop and the flush) into a device array of its
// file that gsplat_debug_read_stamps[_fwd] copies out.  No stamp code exists in the normal build.
#ifndef GS_STAMP
#define GS_STAMP 0
#endif
#if GS_STAMP
#define GS_STAMP_WORDS 16
#define GS_NOW() ((unsigned long long)__builtin_readcyclecounter())
#define GS_LAP(acc) do { const unsigned long long _n = GS_NOW(); (acc) += _n - st_last; st_last = _n; } while (0)
#else
#define GS_LAP(acc) do { } while (0)
#endif
// Backward batch size: 124 slots keep the block at 20 392 B of LDS (records 4 KB, f64 accumulators 9.7 KB, lists + third
// record array 5.8 KB), i.e. EIGHT workgroups per CU (160 KB / 8 = 20 480 B), matching the 64 VGPRs render_bwd_kernel is
// held to: 8 waves per SIMD and 2048 resident workgroups, which 1080p's 8160 tiles fill in 3.98 rounds (r02: 0.350 ->
// 0.342 ms against 128 slots / 72 VGPRs / 7 workgroups per CU).  256 slots (41 KB, 3 blocks/CU) measured 0.76 ms vs
// 0.57 ms when tried in r01, 64 slots 0.63 ms (twice the barriers and per-batch work).
#ifndef GS_BWD_BATCH
#define GS_BWD_BATCH 124
#endif

// Forward batch size: 248 slots keep the block at 20 KB of LDS = EIGHT workgroups per CU at the kernel's 62 VGPRs (256
// slots: 20 800 B, seven).  r02 measured +-0 for this; with r04's shorter loop it is -6 us (profiles/r04_ab_priority...).
#ifndef GS_FWD_BATCH
#define GS_FWD_BATCH 248
#endif
constexpr int kBatch = GS_FWD_BATCH;

template <bool kPacked>
__device__ __forceinline__ SplatRec load_record(int g, const float4 *__restrict__ recs, const RawSplats &raw) {
  if constexpr (kPacked) {
    SplatRec s;
    s.r0 = recs[3 * g]; s.r1 = recs[3 * g + 1]; s.r2 = recs[3 * g + 2];
    return s;
  } else {
    return make_record(raw.uv[2 * g], raw.uv[2 * g + 1], raw.conic[3 * g], raw.conic[3 * g + 1], raw.conic[3 * g + 2],
                       raw.opacity[g], raw.rgb[3 * g], raw.rgb[3 * g + 1], raw.rgb[3 * g + 2]);
  }
}

constexpr int kListStride = kBatch;  // entries per row list (a batch can put all of its 256 slots on one list)

// bit of (wave, row) in the 16-bit block mask: block (bx, by) = ((wave & 1) * 2 + (row & 1), (wave >> 1) * 2 + (row >> 1))
__device__ __forceinline__ int wave_first_bit(int wave) { return (wave >> 1) * 8 + (wave & 1) * 2; }

struct RowCounts { int c0, c1, c2, c3; };

// Compacts, for each of the wave's four rows, the slots of the staged batch that hit the row's block
// (and lie below the row's stop index `lim*` in the backward).  `s_r2`: the record array whose .w holds the 16 block bits
// (the backward's third array, the forward's second).  A list entry is the slot's byte offset into the
// record arrays (slot * 16), so the loop needs no shift; counts are wave-uniform.
template <int kStride>
__device__ __forceinline__ RowCounts build_row_lists(const float4 *s_r2, unsigned short *lists, int count, int wave,
                                                     int lane, int lim0, int lim1, int lim2, int lim3, int round,
                                                     int slot0 = 0) {  // slot0: the record arrays' slot of `s_r2[0]` (r06: two sets)
  RowCounts rc = {0, 0, 0, 0};
  const int b0 = wave_first_bit(wave);
  for (int sb = 0; sb < count; sb += 64) {
    const int slot = sb + lane;
    const unsigned int nib = slot < count ? (__float_as_uint(s_r2[slot].w) >> b0) : 0u;
    const bool h0 = (nib & 1u) && slot < lim0, h1 = (nib & 2u) && slot < lim1;
    const bool h2 = (nib & 16u) && slot < lim2, h3 = (nib & 32u) && slot < lim3;
    const unsigned long long m0 = __ballot(h0), m1 = __ballot(h1), m2 = __ballot(h2), m3 = __ballot(h3);
    if ((m0 | m1 | m2 | m3) == 0ull) continue;
#define GS_MBCNT(m) __builtin_amdgcn_mbcnt_hi((unsigned int)((m) >> 32), __builtin_amdgcn_mbcnt_lo((unsigned int)(m), 0u))
    if (h0) lists[0 * kStride + rc.c0 + GS_MBCNT(m0)] = (unsigned short)((slot0 + slot) << 4);
    if (h1) lists[1 * kStride + rc.c1 + GS_MBCNT(m1)] = (unsigned short)((slot0 + slot) << 4);
    if (h2) lists[2 * kStride + rc.c2 + GS_MBCNT(m2)] = (unsigned short)((slot0 + slot) << 4);
    if (h3) lists[3 * kStride + rc.c3 + GS_MBCNT(m3)] = (unsigned short)((slot0 + slot) << 4);
#undef GS_MBCNT
    rc.c0 += __popcll(m0); rc.c1 += __popcll(m1); rc.c2 += __popcll(m2); rc.c3 += __popcll(m3);
  }
  // Pad the shorter lists up to the wave's trip count (rounded up to `round`) with the sentinel slot kStride, whose
  // record is all zeros (opacity 0 -> alpha 0): a row past the end of its list then needs no "am I active" test.
  const int longest = max(max(rc.c0, rc.c1), max(rc.c2, rc.c3));
  const int padded = (longest + round - 1) / round * round;
  const unsigned short sentinel = (unsigned short)((slot0 + kStride) << 4);
  for (int k = lane; k < padded; k += 64) {
    if (k >= rc.c0) lists[0 * kStride + k] = sentinel;
    if (k >= rc.c1) lists[1 * kStride + k] = sentinel;
    if (k >= rc.c2) lists[2 * kStride + k] = sentinel;
    if (k >= rc.c3) lists[3 * kStride + k] = sentinel;
  }
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_wave_barrier();
  return rc;
}

__device__ __forceinline__ int row_max_int(int v) {  // max over the 16 lanes of a row, in every lane of the row
  v = max(v, __builtin_amdgcn_update_dpp(v, v, 0xB1, 0xF, 0xF, false));
  v = max(v, __builtin_amdgcn_update_dpp(v, v, 0x4E, 0xF, 0xF, false));
  v = max(v, __builtin_amdgcn_update_dpp(v, v, 0x141, 0xF, 0xF, false));
  v = max(v, __builtin_amdgcn_update_dpp(v, v, 0x140, 0xF, 0xF, false));
  return v;
}

// One launch of `kernel`, its arguments converted to its parameter types.  With both events it is a timed launch (the
// context's per-stage timing): the events take the begin and end timestamps of THIS dispatch from its completion signal.
// Two hipEventRecord calls around the launch are barrier packets of their own and kept the GPU idle for ~11 us before and
// ~6 us after the kernel in every step they were on.
template <typename... P>
static void launch_tiles(void (*kernel)(P...), dim3 grid, hipStream_t st, hipEvent_t ev_start, hipEvent_t ev_stop,
                         std::common_type_t<P>... args) {
  if (ev_start && ev_stop) hipExtLaunchKernelGGL(kernel, grid, dim3(256), 0, st, ev_start, ev_stop, 0, args...);
  else kernel<<<grid, dim3(256), 0, st>>>(args...);
}

}  // namespace gs
