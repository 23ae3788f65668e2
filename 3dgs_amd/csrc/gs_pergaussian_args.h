// gs_pergaussian_args.h -- what the per-gaussian launchers take (gs_launch.h: launch_project_cull ... launch_sh_adam_dir;
// defined in gs_preprocess.hip and gs_preprocess_bwd.hip next to their kernels).  Plain pointers and numbers, no context:
// callers start from `{}` and assign by name, as with RenderFwdArgs / RenderBwdArgs (gs_render.h).  The members that
// select a kernel's instantiation are listed last in each struct; a new mode is a member here and a line of the dispatch.
#pragma once
#include "gs_common.h"

namespace gs {

// project_cull_kernel: world -> camera -> pixel -> keep-mask for all N, and the compaction ranks
struct CullArgs {
  const float *xyz, *view, *proj;
  int N, width, height;
  float near_thresh;
  int padding;
  float *xyz_c, *uv;  // [N,3], [N,2] uncompacted; null: not materialised (a lean context)
  unsigned char *mask;
  int *rank, *slice_counts;
  unsigned long long *pair_counters;
  int *kept;         // the slices' kept gaussians as lists, for a compacted walk; else null
  int *chunk_first;  // for sh_colour_kernel beside preprocess_geom_kernel; else null
};

// preprocess_kernel and preprocess_geom_kernel: everything per kept gaussian, written at its compacted slot
struct PreprocessArgs {
  gsplat_gaussians g;
  const float *view, *proj;
  const unsigned char *mask;
  int *rank;
  const int *slice_counts, *kept;
  int width, height, ntx, nty;
  float fx, fy, tan_fovx, tan_fovy, mh_dist, campos[3];
  // out, compacted order (the kernels' PreOut)
  int *c2g;
  float *xyz_c, *uv, *sigma, *conic, *J, *rgb, *radius;
  float4 *recs;
  int *counts;
  unsigned long long *hitmask, *pairs;
  int *table;  // counting-sort route: the per-workgroup tile histograms (the launcher sizes the LDS one); else null
  float *dir_sums;  // launch_preprocess only: [M,9] gs::sh_dir_sums per kept gaussian (preprocess_kernel<.., kDirSums>); else null
  // the form
  int l_max;         // launch_preprocess only
  bool store_mid;    // Sigma, J, conic and colour are stored
  bool compact;      // the walk is over the compacted slots
  bool antialiased;  // launch_preprocess only
};

// sh_colour_kernel (l_max 1..3)
struct ShColourArgs {
  gsplat_gaussians g;
  const unsigned char *mask;
  const int *rank, *chunk_first, *slice_counts, *kept;
  float campos[3];
  float *rgb_out;
  float4 *recs;
  int l_max;
  bool compact;
};

// preprocess_bwd_kernel, and cam_grad_finalize_kernel behind it when cam_rows is set
struct PreprocessBwdArgs {
  gsplat_gaussians g;
  const float *view, *proj;
  int M;
  const int *c2g;
  const float *xyz_c;
  const float4 *rows;
  float fx, fy, tan_fovx, tan_fovy, fwd_tan_fovx, fwd_tan_fovy, mh_dist, campos[3];
  int width, height;
  gsplat_gradients out;    // compacted arrays (the kernels' BwdOut), any of them null
  float *common, *uv_norm;  // split form: rows at the gaussians' global indices instead
  int ranged, first, end;  // ranged: only the gaussians with global index in [first, end)
  int span;                // compacted slots the grid covers (> 0)
  const gsplat_adam_fused *adam;  // with adam_mode != 0: the optimizer state
  float *adam_dir;                // adam_mode 3: [M,3], from sh_adam_dir_kernel
  double *cam_rows;               // camera form: [ceil(span/64),16] partial sums ...
  float *grad_view, *grad_campos;  // ... and where cam_grad_finalize_kernel leaves their totals
  // plain form and adam_mode 1 (no other Adam form, no camera or anti-aliased form): [M,9] the recorded forward's gs::sh_dir_sums, read INSTEAD of the SH
  // rows, band 0 and xyz_c (preprocess_bwd_kernel<.., kDirSums>); null: the kernel reads the rows
  const float *dir_sums;
  // the form
  int l_max;
  int adam_mode;  // 0 none; the kernel's kAdam 1, 2, 3
  bool rows_depth, rows_abs, antialiased;
};

// sh_adam_dir_kernel (l_max 1..3): the SH group's Adam step and the position gradient through the view direction
struct ShAdamDirArgs {
  int M;
  const int *c2g;
  float *sh, *m, *v;
  float lr, b1, b2, eps, bias1, bias2;
  const float *xyz, *band0;
  float campos[3];
  const float4 *rows;
  float *dir_out;
  int l_max;
};

}  // namespace gs
