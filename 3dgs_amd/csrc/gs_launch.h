// gs_launch.h -- the host functions one .hip file of the library defines and another calls, declared once.  The files
// that define them include this header too, so callers and definitions read one text: there is no second copy of a
// prototype to fall behind (a definition whose parameters drift is, to C++, a new overload -- the linker still has the
// last word on that, but the declaration to look at is this one).
#pragma once
#include <type_traits>

#include "gs_common.h"

namespace gs {

struct TileSegments;  // gs_render.h
struct FwdSegments;
struct RenderFwdArgs;
struct RenderBwdArgs;
struct ReplayArgs;
struct CullArgs;  // gs_pergaussian_args.h
struct PreprocessArgs;
struct ShColourArgs;
struct PreprocessBwdArgs;
struct ShAdamDirArgs;

// ---- gs_binning.hip
size_t binning_temp_bytes(size_t N, size_t S, int num_tiles);
int scan_counts(int N, const int *counts, int *offsets, void *temp, size_t temp_bytes, hipStream_t st);
bool binning_supports_counting_sort(int num_tiles);
bool binning_prefers_radix(size_t S, int num_tiles);
bool binning_next_route_is_radix(bool was_counting_sort, size_t S, int num_tiles, long long longest);
size_t binning_table_bytes(int num_tiles);
int binning_offsets(int ntx, int nty, int *table, int *long_tiles, hipStream_t st);
int binning_scatter_and_sort(const float *uv, const float *xyz_c, const float *radius,
                             const unsigned long long *hitmask, const int *rank, int N, int ntx, int nty,
                             const int *table, int *ranges, size_t S, unsigned long long *payload,
                             int *long_tiles, int *sorted_out, long long longest, const int *m_total,
                             const unsigned long long *pair_counters, unsigned long long *pub,
                             unsigned long long ticket, hipStream_t st, const SortFork *fork, bool compact_walk,
                             bool keys_ok);
int emit_sort_ranges(const float *uv, const float *xyz_c, const float *radius, int ntx, int nty, int N,
                     const unsigned char *mask, const int *rank, const int *offsets, size_t S, unsigned int *tkeys_a,
                     unsigned int *tkeys_b, unsigned long long *pay_a, unsigned long long *pay_b, int *sorted_out,
                     int *ranges, void *temp, size_t temp_bytes, hipStream_t st, bool already_emitted,
                     const unsigned long long *hitmask);
int launch_tile_emit(const float *uv, const float *xyz_c, const float *radius, int ntx, int nty, int N,
                     const unsigned char *mask, const int *rank, const int *offsets,
                     const unsigned long long *hitmask, long long capacity, unsigned int *tkeys,
                     unsigned long long *payload, hipStream_t st);

// ---- gs_render_fwd.hip, gs_render_bwd.hip.  The two compositing launchers take their arguments by name (gs_render.h:
// RenderFwdArgs, RenderBwdArgs).  launch_render_bwd stamps ev_start / ev_stop from the dispatch itself when both are
// given, whichever kernel it selects (until the argument structs only the packed-records-and-rows forms did; no caller
// times another).
int launch_render_fwd(const RenderFwdArgs &a, hipStream_t st);
int launch_fwd_segments_table(const int *ranges, int num_tiles, const FwdSegments &fs, hipStream_t st);
int launch_render_bwd(const RenderBwdArgs &a, hipStream_t st);
int launch_tile_segments(const int *ranges, const int *tops, int num_tiles, const TileSegments &seg, hipStream_t st);
int launch_tile_order(const int *work, const int *ranges, int num_tiles, int *order, hipStream_t st);
bool tile_order_supported(int num_tiles);

// ---- gs_replay.hip: the kernels that walk a recorded forward again (gs_render.h: ReplayArgs)
int launch_contributions(const ReplayArgs &a, float *weight_sum, float *weight_max, int *pixels, hipStream_t st);
// per pixel the list position of the first composited entry behind which T <= threshold and that gaussian's z from the
// compacted xyz_c [M,3] (median_depth_kernel): depth [H,W], index [H,W] or null; (0, -1) where T never gets there
int launch_median_depth(const ReplayArgs &a, const float *xyz_c, float threshold, float *depth, int *index, hipStream_t st);
// the caller's channels through the recorded forward's weights and back (features_fwd_kernel, features_lift_kernel):
// features [N,C] in global order -> out [H,W,C]; map [H,W,C] -> lifted [N,C] in global order, accumulated into
int launch_features_fwd(const ReplayArgs &a, int channels, const float *features, float *out, hipStream_t st);
int launch_features_lift(const ReplayArgs &a, int channels, const float *map, float *lifted, hipStream_t st);
// the feature map's gradient with respect to the geometry (features_bwd_kernel): features [N,C] in global order and
// grad_map [H,W,C] -> columns 3..8 (opacity logit, conic, uv) of the gradient rows [M,16], added to what they hold
int launch_features_bwd(const ReplayArgs &a, int channels, const float *features, const float *grad_map, float *rows,
                        hipStream_t st);

// ---- gs_filter3d.hip: the 3D smoothing filter's parameter transform and its chain rule (gsplat_context_set_filter3d)
int launch_filter3d_apply(const float *scale, const float *opacity, const float *filter3d, int N, float *scale_eff,
                          float *opacity_eff, hipStream_t st);
int launch_filter3d_apply_bwd(const float *scale, const float *opacity, const float *filter3d, const int *rows, int M,
                              float *grad_scale, int scale_stride, float *grad_opacity, int opacity_stride,
                              bool at_gaussian, int first, int end, int span, hipStream_t st);

// ---- gs_preprocess.hip: the per-gaussian forward.  Arguments by name (gs_pergaussian_args.h); each launcher selects its
// kernel's instantiation from the form members and writes the kernel's argument list once.
int launch_project_cull(const CullArgs &a, hipStream_t st);
int launch_preprocess(const PreprocessArgs &a, hipStream_t st);  // form: (l_max, store_mid, compact, antialiased)
// the two-kernel forward; the fork / join of the side-by-side form stays with the caller.  colour: 0 degree 0, formed by the
// geometry kernel; 1 read from a.rgb, where sh_colour_kernel has left it; 2 written into the records by sh_colour_kernel
int launch_sh_colour(const ShColourArgs &a, hipStream_t st);                         // form: (l_max 1..3, compact)
int launch_preprocess_geom(const PreprocessArgs &a, int colour, hipStream_t st);    // form: (colour, store_mid, compact)
size_t scan_counts_temp_bytes(size_t N);  // rocPRIM's exclusive scan over N + 1 counts (gs_binning.hip: scan_counts)
int launch_publish_counts(const int *rank_total, const int *offsets_total, const unsigned long long *pair_counters,
                          unsigned long long *pub, unsigned long long ticket, hipStream_t st);

// ---- gs_preprocess_bwd.hip: the per-gaussian backward; launches cam_grad_finalize_kernel too when a.cam_rows is set
int launch_preprocess_bwd(const PreprocessBwdArgs &a, hipStream_t st);
int launch_sh_adam_dir(const ShAdamDirArgs &a, hipStream_t st);  // (l_max 1..3)

// ---- gs_exchange.hip: the compositing backward's colour rows scattered to global order (gsplat_backward_render_depth)
int launch_scatter_rgb_rows(const unsigned char *mask, const int *rank, int N, const float *rows, float *rgb_global,
                            float *common, float *uv_norm, hipStream_t st);

// ---- run-time switches as compile-time constants, for the launchers' dispatches: f is a generic lambda that names the
// kernel's instantiation from the constant's type (decltype(x)::value) -- no macro, one argument list per kernel
template <class F>
void with_bool(bool b, F &&f) {
  if (b) f(std::true_type{}); else f(std::false_type{});
}
// SH degree kLowest..3 (a degree outside the range takes 3, as the switch statements this replaces did)
template <int kLowest, class F>
void with_degree(int l_max, F &&f) {
  static_assert(kLowest == 0 || kLowest == 1, "kernels exist from degree 0 or from degree 1");
  if constexpr (kLowest == 0) {
    if (l_max == 0) return f(std::integral_constant<int, 0>{});
  }
  if (l_max == 1) f(std::integral_constant<int, 1>{});
  else if (l_max == 2) f(std::integral_constant<int, 2>{});
  else f(std::integral_constant<int, 3>{});
}

}  // namespace gs
