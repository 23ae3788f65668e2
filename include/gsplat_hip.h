/*
 * gsplat_hip.h -- C ABI of libgsplat_hip.so, the MI355X (gfx950) differentiable
 * gaussian-splat rasterizer.
 *
 * Drop-in boundary.  Every gsplat_<op> below replaces the free function <op> that the
 * reference declares in include/gsplat_cuda/cuda_forward.cuh:26-131 and
 * include/gsplat_cuda/cuda_backward.cuh:21-123 (AndrewBoessen/3DGS) and takes the same
 * raw device pointers and scalars in the same order.  ABI adaptations, all mechanical:
 *   float3 campos        -> three floats
 *   float4* radius       -> float* (4 floats per gaussian, 16-byte aligned)
 *   bool* mask           -> unsigned char* (one byte per gaussian, 0/1)
 *   size_t& count        -> size_t*
 *   cudaStream_t stream  -> void* (a hipStream_t; NULL = the null stream)
 *   void / exit(1)       -> int status (0 = GSPLAT_OK, negative = error; nothing exits)
 * include/gsplat_cuda/cuda_forward.cuh and cuda_backward.cuh in this repository are C++
 * shims with the reference's exact signatures (and its print-and-exit error behaviour)
 * that forward to these symbols, so a host written against the reference's headers
 * compiles unchanged.
 *
 * Ownership: the caller owns every buffer it passes.  Outputs documented "+=" are
 * accumulated into and must be pre-zeroed by the caller, exactly as in the reference
 * (cuda/trainer.cu:247-261).  Operators may use library-owned scratch memory that is
 * grown on demand and released by gsplat_release_scratch().
 *
 * Threading: the stand-alone operators are written for one host thread per device at a time (the reference's trainer
 * thread).  A gsplat_context is used by one thread at a time; different contexts may be driven by different threads
 * of one process on the same stream (several in-process ranks, 3dgs_amd/dist.py ThreadGroup): the entry points that
 * touch the library-owned scratch (gsplat_fused_loss, gsplat_compute_psnr, gsplat_compact/scatter_masked_array,
 * gsplat_get_sorted_gaussian_list, gsplat_initialize_gaussians, gsplat_knn_mean_distance) serialise on a lock.
 */
#ifndef GSPLAT_HIP_H
#define GSPLAT_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GSPLAT_OK 0
#define GSPLAT_ERR_NULL_POINTER (-1)   /* a required pointer is NULL            (checks.cuh:17-21)  */
#define GSPLAT_ERR_NOT_DEVICE (-2)     /* pointer is not device memory          (checks.cuh:23-38)  */
#define GSPLAT_ERR_INVALID_ARG (-3)    /* negative size, l_max outside 0..3 ... (raster.cu:58-60)   */
#define GSPLAT_ERR_HIP (-4)            /* a HIP runtime call or kernel launch failed                 */
#define GSPLAT_ERR_NO_VISIBLE (-5)     /* nothing survives culling              (raster.cu:38-41)   */
#define GSPLAT_ERR_CAPACITY (-6)       /* context capacity exceeded                                   */

#define GSPLAT_TILE_SIZE 16 /* TILE_SIZE_FWD / TILE_SIZE_BWD, cuda_forward.cuh:8, cuda_backward.cuh:8 */

/* Human-readable text for the last error raised on the calling thread. */
const char *gsplat_last_error(void);
/* Library ABI version (bumped when a signature changes); bindings compare it with the GSPLAT_ABI_VERSION they were
 * written against, so a stale prebuilt library fails at load time, not with a wrong argument list. */
#define GSPLAT_ABI_VERSION 9
int gsplat_abi_version(void);
/* What the loaded binary was built from: sha256 (first 16 hex digits) over the kernel sources (3dgs_amd/csrc: Makefile,
 * *.h, *.hip) at link time, and the extra compiler flags of a diagnostic build ("" for the product build).  A loader
 * that did not build the library itself compares the hash with the sources it sees (3dgs_amd/_lib.py), and stored
 * profiles (profiles/traffic.json) are tied to it. */
const char *gsplat_source_hash(void);
const char *gsplat_build_flags(void);
/* Frees library-owned scratch memory of the current device. */
int gsplat_release_scratch(void);

/* Device block pool.  The reference host creates and destroys ~20 thrust::device_vectors per training iteration (a
 * fresh ForwardPassData, cuda/trainer.cu:1295; one vector per compact_masked_array, cuda/trainer.cu:941-964,1028-1044):
 * with the runtime's allocator every one of them is a hipMalloc + a hipFree (which synchronises the device) -- 4 of the
 * 6.5 ms the unmodified reference-host iteration took at 1e6 gaussians.  The vectors the drop-in headers create
 * (include/gsplat_cuda/cuda_data.cuh: gsplat_shim::device_array) draw from this pool instead: a freed block is kept and
 * handed to the next request of its size class (three mantissa bits: <= 12.5 % slack), so the steady state allocates
 * nothing.  Blocks are reused in STREAM ORDER: a block freed while work of stream s still reads it is first re-used by
 * work queued on s afterwards; a request from another stream is ordered behind s (r06: the _on forms below).
 * gsplat_pool_release hipFree()s the idle blocks; gsplat_pool_bytes reports idle (idle_only != 0) or idle + live bytes. */
int gsplat_pool_alloc(void **ptr, size_t bytes);
int gsplat_pool_free(void *ptr);
/* r06: the stream-aware forms.  gsplat_pool_free_on(ptr, s): work queued on stream `s` so far may still touch the block.
 * gsplat_pool_alloc_on(&ptr, bytes, t): the block will next be touched by work queued on stream `t`; when it takes a
 * block that another stream returned, `t` is first ordered behind that stream (an event recorded on it now -- later than
 * the return, hence covering it -- and awaited by `t`; a device synchronisation if that stream no longer exists); blocks
 * returned by `t` itself are preferred and cost nothing.  The plain forms above are the NULL-stream forms
 * (cuda/trainer.cu: everything but the image upload runs on the NULL stream; its transfer_stream, :1257-1259, is the
 * reason the pool needs the ordering).  gsplat_pool_cross_stream_reuses: how often the ordering was needed. */
int gsplat_pool_alloc_on(void **ptr, size_t bytes, void *stream);
int gsplat_pool_free_on(void *ptr, void *stream);
unsigned long long gsplat_pool_cross_stream_reuses(void);
int gsplat_pool_release(void);
/* Frees idle blocks of the CURRENT device (largest first) while more than keep_bytes of them are cached; other devices
 * are neither synchronised nor touched.  What gsplat_context_destroy calls (keep_bytes = 1 GiB). */
int gsplat_pool_trim(size_t keep_bytes);
size_t gsplat_pool_bytes(int idle_only);

/* ---------------------------------------------------------------- forward operators --- */

/* replaces compute_camera_space_points  (cuda_forward.cuh:50-51, cuda/projection.cu:100-114)
 * xyz_c[N,3] = view[0:3,0:4] * [xyz_w;1], view row-major 4x4 */
int gsplat_compute_camera_space_points(const float *xyz_w, const float *view, int N, float *xyz_c, void *stream);

/* replaces project_to_screen  (cuda_forward.cuh:63-64, cuda/projection.cu:116-130) -> uv[N,2] */
int gsplat_project_to_screen(const float *xyz, const float *proj, int N, int width, int height, float *uv,
                             void *stream);

/* replaces cull_gaussians  (cuda_forward.cuh:78-79, cuda/culling.cu:361-375); mask: 1 = keep */
int gsplat_cull_gaussians(const float *uv, const float *xyz, int N, float near_thresh, int padding, int width,
                          int height, unsigned char *mask, void *stream);

/* replaces compute_sigma  (cuda_forward.cuh:39, cuda/gaussian.cu:220-235)
 * quaternion[N,4] in (w,x,y,z) order, scale[N,3] log-scales -> sigma[N,6] = [xx,xy,xz,yy,yz,zz] */
int gsplat_compute_sigma(const float *quaternion, const float *scale, int N, float *sigma, void *stream);

/* replaces compute_conic  (cuda_forward.cuh:26-28, cuda/gaussian.cu:237-262)
 * -> J[N,6], conic[N,3] = [c00,c01,c11], radius[N,4] = {r_major, r_minor, sin(theta), cos(theta)} */
int gsplat_compute_conic(const float *xyz, const float *view, const float *sigma, float focal_x, float focal_y,
                         float tan_fovx, float tan_fovy, float mh_dist, int N, float *J, float *conic,
                         float *radius, void *stream);

/* replaces get_sorted_gaussian_list  (cuda_forward.cuh:95-97, cuda/culling.cu:386-475)
 * Two-call protocol, as in the reference:
 *   sorted_gaussians == NULL : *sorted_gaussian_count <- number of coarse (tile, gaussian)
 *                              candidate pairs; the caller sizes sorted_gaussians with it.
 *   sorted_gaussians != NULL : sorted_gaussians[0..S) <- gaussian ids ordered by (tile, depth),
 *                              ties by gaussian id; splat_start_end_idx_by_tile_idx[0..T] <-
 *                              start offsets (entry T = S).  Blocks the host, as the reference does. */
int gsplat_get_sorted_gaussian_list(const float *uv, const float *xyz, const float *radius, int n_tiles_x,
                                    int n_tiles_y, int N, size_t *sorted_gaussian_count, int *sorted_gaussians,
                                    int *splat_start_end_idx_by_tile_idx, void *stream);

/* replaces precompute_spherical_harmonics  (cuda_forward.cuh:111-113, cuda/spherical_harmonics.cu:62-94)
 * sh_coefficients[N,(l_max+1)^2-1,3] (may be NULL when l_max == 0), band 0 in sh_coeffs_band_0[N,3];
 * rgb = 0.5 + sum coeff * Y(dir), dir = normalize(xyz - campos); no clamp */
int gsplat_precompute_spherical_harmonics(const float *xyz, const float *sh_coefficients,
                                          const float *sh_coeffs_band_0, float campos_x, float campos_y,
                                          float campos_z, int l_max, int N, float *rgb, void *stream);

/* replaces render_image  (cuda_forward.cuh:131-134, cuda/render.cu:110-135)
 * -> splats_per_pixel[H,W], weight_per_pixel[H,W] (final transmittance), image[H,W,3] */
int gsplat_render_image(const float *uv, const float *opacity, const float *conic, const float *rgb,
                        float background_opacity, const int *sorted_splats, const int *splat_range_by_tile,
                        int image_width, int image_height, int *splats_per_pixel, float *weight_per_pixel,
                        float *image, void *stream);

/* --------------------------------------------------------------- backward operators --- */

/* replaces project_to_screen_backward  (cuda_backward.cuh:21-23); xyz_c_grad_in += */
int gsplat_project_to_screen_backward(const float *xyz_c, const float *proj, const float *uv_grad_out, int N,
                                      int width, int height, float *xyz_c_grad_in, void *stream);

/* replaces compute_camera_space_points_backward  (cuda_backward.cuh:34-36); xyz_w_grad_in += */
int gsplat_compute_camera_space_points_backward(const float *xyz_w, const float *view, const float *xyz_c_grad_out,
                                                int N, float *xyz_w_grad_in, void *stream);

/* replaces compute_projection_jacobian_backward  (cuda_backward.cuh:47-49); xyz_c_grad_in += */
int gsplat_compute_projection_jacobian_backward(const float *xyz_c, float focal_x, float focal_y, float tan_fovx,
                                                float tan_fovy, const float *J_grad_out, int N,
                                                float *xyz_c_grad_in, void *stream);

/* replaces compute_conic_backward  (cuda_backward.cuh:61-63); J_grad_in +=, sigma_grad_in +=
 * (off-diagonal sigma entries receive the sum of both symmetric positions) */
int gsplat_compute_conic_backward(const float *J, const float *sigma, const float *view, const float *conic,
                                  const float *conic_grad_out, int N, float *J_grad_in, float *sigma_grad_in,
                                  void *stream);

/* replaces compute_sigma_backward  (cuda_backward.cuh:75-76); quaternion_grad_in =, scale_grad_in = */
int gsplat_compute_sigma_backward(const float *quaternion, const float *scale, const float *sigma_grad_out, int N,
                                  float *quaternion_grad_in, float *scale_grad_in, void *stream);

/* replaces precompute_spherical_harmonics_backward  (cuda_backward.cuh:90-94)
 * sh_grad_in =, sh_grad_band_0_in =, xyz_c_grad_in += */
int gsplat_precompute_spherical_harmonics_backward(const float *xyz_c, const float *rgb_vals,
                                                   const float *sh_coeffs, float campos_x, float campos_y,
                                                   float campos_z, const float *rgb_grad_out, int l_max, int N,
                                                   float *sh_grad_in, float *sh_grad_band_0_in,
                                                   float *xyz_c_grad_in, void *stream);

/* replaces render_image_backward  (cuda_backward.cuh:116-122); all four outputs += (pre-zeroed by the caller);
 * grad_uv carries the reference's extra 0.5*W / 0.5*H factor (cuda/render_backward.cu:186-187) */
int gsplat_render_image_backward(const float *uvs, const float *opacity, const float *conic, const float *rgb,
                                 float background_opacity, const int *sorted_splats,
                                 const int *splat_range_by_tile, const int *num_splats_per_pixel,
                                 const float *final_weight_per_pixel, const float *grad_image, int image_width,
                                 int image_height, float *grad_rgb, float *grad_opacity, float *grad_uv,
                                 float *grad_conic, void *stream);

/* ---------------------------------------------------- "next" rows: loss, metric, optimizer --- */

/* replaces fused_loss  (cuda_forward.cuh:146-147, cuda/loss.cu:430-471): L1 + SSIM loss and dL/dimage.
 * image_grad[H,W,3] is overwritten.  If loss_out != NULL the mean loss is read back (blocks the host, as the
 * reference's return value does); pass NULL to stay asynchronous. */
int gsplat_fused_loss(const float *predicted_data, const float *gt_data, int rows, int cols, float ssim_weight,
                      float *image_grad, float *loss_out, void *stream);

/* replaces compute_psnr  (cuda_forward.cuh:158, cuda/loss.cu:510-525); blocks the host */
int gsplat_compute_psnr(const float *predicted_data, const float *gt_data, int rows, int cols, float *psnr_out,
                        void *stream);

/* replaces adam_step  (include/gsplat_cuda/optimizer.cuh:27-29, cuda/optimizer.cu:31-44) on N*S elements */
int gsplat_adam_step(float *params, const float *param_grads, float *exp_avg, float *exp_avg_sq, float lr, float b1,
                     float b2, float eps, float bias1, float bias2, int N, int S, void *stream);

/* One Adam parameter group: global-order parameter and moment arrays [N,stride] and its learning rate. */
#define GSPLAT_MAX_ADAM_GROUPS 8
typedef struct gsplat_adam_group {
  float *param;             /* [N,stride] device, updated in place                                  */
  float *exp_avg;           /* [N,stride] device, first moment                                      */
  float *exp_avg_sq;        /* [N,stride] device, second moment                                     */
  const float *grad;        /* [M,stride] device, compacted order (gsplat_optimizer_step only)      */
  int stride;
  int packed_column;        /* first column in a packed row (gsplat_optimizer_step_packed only)     */
  float lr;
} gsplat_adam_group;

/* replaces TrainerImpl::optimizer_step  (cuda/trainer.cu:1027-1158): the reference compacts parameters and both
 * moments of every group by the view's mask, runs adam_step on the compacted copies and scatters them back
 * (~35 thrust passes).  Here one kernel updates the visible rows in place through compact_to_global
 * (gsplat_forward_view.compact_to_global, length num_culled); rows the view did not see keep their moments.
 * If uv_grad_accum / grad_accum_dur are non-NULL the densification statistics of trainer.cu:1136-1157 are
 * updated too: uv_grad_accum[i] += |grad_uv[r]|, grad_accum_dur[i] += 1. */
int gsplat_optimizer_step(const int *compact_to_global, int num_culled, const gsplat_adam_group *groups, int n_groups,
                          float b1, float b2, float eps, float bias1, float bias2, const float *grad_uv,
                          float *uv_grad_accum, int *grad_accum_dur, void *stream);

/* The spherical-harmonics group of gsplat_optimizer_step without its gradient array.  The SH gradients of ONE view are an
 * outer product (cuda/spherical_harmonics_backward.cu:168-209): d/d sh[k][c] = Y_{k+1}(direction) * grad_precompute_rgb[c],
 * direction = normalised (xyz - camera position) -- the values the backward would have stored in grad_sh, bit for bit
 * (the same basis function, the same product).  For the visible rows (compact_to_global, num_culled) this entry point
 * rebuilds them from the 24 bytes they are made of and applies the same in-place Adam update to sh / exp_avg /
 * exp_avg_sq [N, (l_max+1)^2 - 1, 3]; a backward that was given grad_sh == NULL plus this call replace a backward that
 * writes grad_sh and an optimizer group that reads it back (360 bytes per visible gaussian and step at l_max 3).
 * xyz [N,3] must still hold the positions the backward saw: call it BEFORE the step that updates the xyz group.
 * grad_precompute_rgb [num_culled,3]: the intermediate gradient of that name (gsplat_gradients). */
int gsplat_optimizer_step_sh_factored(const int *compact_to_global, int num_culled, int l_max, float *sh, float *exp_avg,
                                      float *exp_avg_sq, float lr, float b1, float b2, float eps, float bias1,
                                      float bias2, const float *xyz, float cam_x, float cam_y, float cam_z,
                                      const float *grad_precompute_rgb, void *stream);

/* r05 -- the colour groups of a W-view step without their gradient arrays: the band-0 group (rgb[N,3]) and the SH group
 * (sh[N,(l_max+1)^2-1,3]) are updated in place from what the split exchange delivers -- rgb_all = W blocks of
 * `rank_stride` floats, block r = rank r's g_rgb[N,3] in global order followed by its camera position[3] -- as
 * grad[k][c] = sum over the views r (in rank order) of g_rgb^r[c] * Y_k(direction from camera r to the gaussian): the
 * sums gsplat_unpack_gradients_split writes into the packed rows, formed in the same order with the same operations, so
 * parameters and moments are bit-identical to gsplat_unpack_gradients_split + gsplat_optimizer_step_packed -- without
 * writing and re-reading packed[N, 12 + 3 n] (240 B per gaussian at SH degree 3, each way).  A row is updated when
 * common[i*12 + 11], the number of views that saw the gaussian, is positive (the reference's per-view masks,
 * cuda/trainer.cu:1028-1085).  Must run BEFORE the xyz group moves (the directions are rebuilt from xyz).  The other
 * four groups: gsplat_optimizer_step_packed on common[N,12] itself (width 12, columns xyz 0, opacity 3, scale 4,
 * quaternion 7).  sh may be NULL at l_max == 0. */
int gsplat_optimizer_step_sh_views(int l_max, int num_gaussians, int world_size, const float *xyz, const float *rgb_all,
                                   size_t rank_stride, const float *common, float *rgb, float *rgb_exp_avg,
                                   float *rgb_exp_avg_sq, float lr_rgb, float *sh, float *sh_exp_avg,
                                   float *sh_exp_avg_sq, float lr_sh, float b1, float b2, float eps, float bias1,
                                   float bias2, void *stream);

/* Multi-view variant: gradients are rows of the all-reduced packed layout
 * (gsplat_pack_gradients_global / gsplat_unpack_gradients_factored, row width `width`, last column = number of
 * views that saw the gaussian); rows with a zero count are skipped, which is the union of the per-view masks.
 * Densification statistics of a W-view step (trainer.cu:1136-1157 once per view): when uv_grad_accum / grad_accum_dur
 * are non-NULL, uv_grad_accum[i] += uv_norm_sum[i] (the all-reduced gsplat_pack_uv_grad_norm column: the sum over the
 * step's views of |grad_uv|) and grad_accum_dur[i] += the row's view count. */
int gsplat_optimizer_step_packed(const float *packed, int num_gaussians, int width, const gsplat_adam_group *groups,
                                 int n_groups, float b1, float b2, float eps, float bias1, float bias2,
                                 const float *uv_norm_sum, float *uv_grad_accum, int *grad_accum_dur, void *stream);

/* replaces Gaussians::Initialize  (src/gaussian.cpp:38-104; host kd-tree + OpenMP in the reference): the initial
 * gaussians of a sparse point cloud, computed on the GPU.  points_xyz [N,3] doubles and points_rgb [N,3] bytes are
 * DEVICE arrays (COLMAP's Point3D fields, include/gsplat_host.h reads them); outputs are the GaussianParameters
 * arrays: xyz [N,3], rgb [N,3] = (rgb/255 - 0.5)/C0, opacity [N] = logit(0.2), scale [N,3] = log(mean distance to the
 * 3 nearest neighbours, 0.01 if there is none), quaternion [N,4] = (1,0,0,0).  Blocks the host (two small
 * read-backs size the grid). */
int gsplat_initialize_gaussians(const double *points_xyz, const unsigned char *points_rgb, int N, float *xyz, float *rgb,
                                float *opacity, float *scale, float *quaternion, void *stream);
/* the exact k-nearest-neighbour statistic on its own: mean_dist[i] = mean distance of point i to its k (1..8)
 * nearest other points (duplicates count as neighbours at distance 0, as in the reference's kd-tree query) */
int gsplat_knn_mean_distance(const double *points_xyz, int N, int k, float *mean_dist, void *stream);

/* replaces compute_morton_codes  (cuda_forward.cuh:174-188, cuda/culling.cu:14-63): 63-bit Morton code of each
 * position inside the given box, bit-exact with the reference (including its bit-spread masks). */
int gsplat_compute_morton_codes(int N, const float *xyz, float x_max, float y_max, float z_max, float x_min,
                                float y_min, float z_min, unsigned long long *codes, void *stream);

/* replaces clone_gaussians  (adaptive_density.cuh:9-31, cuda/adaptive_density.cu:12-66): gaussians with mask[i] set
 * are copied to row write_ids[i] (exclusive scan of the mask) of the output arrays.  mask is one byte per gaussian. */
int gsplat_clone_gaussians(int N, int num_sh_coef, const unsigned char *mask, const int *write_ids, const float *xyz_in,
                           const float *rgb_in, const float *op_in, const float *scale_in, const float *quat_in,
                           const float *sh_in, float *xyz_out, float *rgb_out, float *op_out, float *scale_out,
                           float *quat_out, float *sh_out, void *stream);

/* replaces split_gaussians  (adaptive_density.cuh:33-57, cuda/adaptive_density.cu:68-164): every masked gaussian
 * yields two gaussians at rows 2*write_ids[i] and 2*write_ids[i]+1: centres drawn from N(xyz, R diag(exp(scale))^2 R^T),
 * scales log(exp(scale)/scale_factor), everything else copied.  `seed` makes the draw reproducible (the reference
 * seeds from time(NULL); its C++ shim passes that). */
int gsplat_split_gaussians(int N, float scale_factor, int num_sh_coef, const unsigned char *mask, const int *write_ids,
                           const float *xyz_in, const float *rgb_in, const float *op_in, const float *scale_in,
                           const float *quat_in, const float *sh_in, float *xyz_out, float *rgb_out, float *op_out,
                           float *scale_out, float *quat_out, float *sh_out, unsigned long long seed, void *stream);

/* The data-parallel half of TrainerImpl::adaptive_density_step (cuda/trainer.cu:416-575): per gaussian the average
 * screen-space gradient uv_grad_accum / grad_accum_dur, the largest extent max(exp(scale)), and the reference's
 * IdentifyPrune / IdentifyClone / IdentifySplit / CombineMasks decisions.  counts[3] (device) receives the number of
 * pruned, cloned and split gaussians.  Masks are one byte per gaussian. */
int gsplat_density_masks(int N, const float *opacity, const float *scale, const float *uv_grad_accum,
                         const int *grad_accum_dur, float op_threshold, float max_scale, float uv_grad_threshold,
                         float clone_scale_threshold, unsigned char *prune_mask, unsigned char *clone_mask,
                         unsigned char *split_mask, unsigned char *keep_mask, int *counts, void *stream);

/* add_sh_band's re-layout (cuda/trainer.cu:363-413): sh_in [N,(l+1)^2-1,3] -> sh_out [N,(l+2)^2-1,3], new
 * coefficients zero.  l_max_old == 0 just zero-fills the first band. */
int gsplat_expand_sh(int N, int l_max_old, const float *sh_in, float *sh_out, void *stream);

/* sort_gaussians' gather (cuda/trainer.cu:793-851): out[i, :] = in[order[i], :] for rows of `stride` floats. */
int gsplat_gather_rows(int N, int stride, const int *order, const float *in, float *out, void *stream);

/* ---- MCMC densification ("3D Gaussian Splatting as Markov Chain Monte Carlo", Kheradmand et al. 2024; gsplat's
 * MCMCStrategy): the four data-parallel pieces; the schedule is the host's (3dgs_amd/trainer.py, config key mcmc).
 * Random numbers come from split_gaussians' counter-based generator: with
 *   bits(seed, c) = splitmix64(splitmix64(seed) ^ (c * 0xD1342543DE82EF95 + 1))
 * the uniform u(seed, c) = (double)(bits >> 11) * 2^-53 lies in [0, 1) and the normals are split_gaussians'.  A seed
 * reproduces every call bit for bit.  N == 0 (K == 0, M == 0) returns GSPLAT_OK without a launch.
 *
 *   gsplat_sample_by_weight  cdf[N]: the inclusive prefix sum of non-negative weights, in double, device memory.  For
 *                            k < K: t = min(u(seed, k) * cdf[N-1], nextafter(cdf[N-1], 0)), samples[k] = the smallest i
 *                            with cdf[i] > t (a row of weight zero is never returned), counts[samples[k]] += 1 (integer
 *                            atomics; counts[N] is accumulated into: the caller clears it).  cdf[N-1] > 0 is checked on
 *                            the device: when it does not hold, nothing is written.
 *   gsplat_mcmc_relocate     in place on the opacity logits [N] and log-scales [N,3]: row i with counts[i] > 0 becomes
 *                            one of n = min(counts[i] + 1, 51) coincident gaussians that together render what it
 *                            rendered: o = sigmoid(logit), o' = 1 - (1 - o)^(1/n),
 *                            den = sum_{i=1..n} sum_{k=0..i-1} C(i-1, k) (-1)^k o'^(k+1) / sqrt(k+1),
 *                            log-scale += log(o / den), logit = logit(clamp(o', min_opacity, 1 - 2^-23)); evaluated in
 *                            double (gsplat: float32) and rounded once.  Rows with counts[i] <= 0 are not written.
 *                            0 < min_opacity < 1.
 *   gsplat_mcmc_add_noise    xyz[i] += Sigma nu in float, Sigma = R diag(exp(scale))^2 R^T with R from the normalised
 *                            quaternion as in split_gaussians, nu_a = normal(seed, 3 i + a) * g * scaler, the gate
 *                            g = 1 / (1 + exp(100 (sigmoid(opacity) - 0.005))): opaque gaussians stay where they are.
 *                            A row with g * scaler == 0 keeps its bits (scaler == 0: all of xyz).
 *   gsplat_mcmc_regularize   the gradient of w_opacity * sum sigmoid(opacity) + w_scale * sum exp(scale), added to
 *                            compacted gradient rows: for j < M, i = compact_to_global[j] (trusted, like the optimizer
 *                            step's), grad_opacity[j] += w_opacity * s (1 - s), grad_scale[3 j + a] += w_scale *
 *                            exp(scale[3 i + a]).  NOTE the difference from gsplat, which regularises and steps every
 *                            gaussian in every iteration: the Adam of this library is masked by visibility, so the
 *                            term reaches only the rows the iteration's view saw. */
int gsplat_sample_by_weight(const double *cdf, int N, int K, unsigned long long seed, int *samples, int *counts,
                            void *stream);
int gsplat_mcmc_relocate(int N, float *opacity, float *scale, const int *counts, float min_opacity, void *stream);
int gsplat_mcmc_add_noise(int N, float *xyz, const float *opacity, const float *scale, const float *quaternion,
                          float scaler, unsigned long long seed, void *stream);
int gsplat_mcmc_regularize(int M, const int *compact_to_global, const float *opacity, const float *scale,
                           float w_opacity, float w_scale, float *grad_opacity, float *grad_scale, void *stream);

/* ------------------------------------------------------------- compaction templates --- */

/* replaces compact_masked_array<STRIDE>  (cuda_data.cuh:106-127): stable compaction of src[N,stride] by mask[N]
 * into dst (room for N*stride floats, or for the selected rows when the caller knows their number, as the reference's
 * callers do: they pass num_culled).  num_selected != NULL: *num_selected <- rows kept (a host value: blocks the host);
 * NULL: no read-back, the call stays asynchronous. */
int gsplat_compact_masked_array(const float *src, const unsigned char *mask, int N, int stride, float *dst,
                                int *num_selected, void *stream);
/* The same with the room of dst stated (r05): rows whose compacted slot is >= dst_rows are NOT written.  The reference's
 * template trusts its caller's num_culled (cuda_data.cuh:106-127) and so do the callers here (no count read-back), but a
 * count that is too small then drops rows instead of overwriting whatever follows dst. */
int gsplat_compact_masked_array_bounded(const float *src, const unsigned char *mask, int N, int stride, float *dst,
                                        int dst_rows, int *num_selected, void *stream);

/* replaces scatter_masked_array<STRIDE>  (cuda_data.cuh:150-167): dst[i] <- src[rank(i)] where mask[i] */
int gsplat_scatter_masked_array(const float *src, const unsigned char *mask, int N, int stride, float *dst,
                                void *stream);

/* --------------------------------------------------- fused per-view pass (additive API) --- */
/*
 * gsplat_rasterize_image / gsplat_backward_pass are the device-resident equivalents of
 * rasterize_image (raster.cuh:22-24, cuda/raster.cu:12-136) and of the operator chain in
 * TrainerImpl::backward_pass (cuda/trainer.cu:941-1012).  They run on a context that owns
 * a persistent workspace (no per-call allocation), fuse the per-gaussian operators into
 * one preprocess kernel each way, and need one host read-back per forward (M and S).
 * Results are identical in layout to ForwardPassData / GaussianGradients: per-gaussian
 * buffers are in compacted (post-cull) order.
 */
typedef struct gsplat_context gsplat_context;

typedef struct gsplat_camera {
  int width, height;
  float focal_x, focal_y;  /* camera.params[0], params[1]                         */
  float campos[3];         /* Image::CamPos()                                     */
  const float *view;       /* device, 16 floats row-major [R|t]  (trainer.cu:1321-1331) */
  const float *proj;       /* device, 16 floats row-major        (trainer.cu:1310-1318) */
} gsplat_camera;

typedef struct gsplat_gaussians {      /* GaussianParameters, cuda_data.cuh:11-16; all device pointers */
  int num_gaussians;
  const float *xyz;        /* [N,3] */
  const float *rgb;        /* [N,3]  SH band 0 */
  const float *sh;         /* [N,(l_max+1)^2-1,3], may be NULL when l_max == 0 */
  const float *opacity;    /* [N]   logits */
  const float *scale;      /* [N,3] log-scales */
  const float *quaternion; /* [N,4] (w,x,y,z) */
} gsplat_gaussians;

typedef struct gsplat_raster_config {  /* the ConfigParameters fields the path reads, raster.cu:33,100 */
  float near_thresh, mh_dist;
  int cull_mask_padding;
} gsplat_raster_config;

typedef struct gsplat_forward_view {   /* ForwardPassData, cuda_data.cuh:70-86: pointers INTO the context */
  size_t num_culled;                   /* M */
  size_t num_pairs;                    /* coarse candidates (what call 1 of get_sorted_gaussian_list reports) */
  size_t num_splats;                   /* S */
  const unsigned char *mask;           /* [N] */
  const float *uv, *xyz_c;             /* [N,2], [N,3] uncompacted */
  const int *compact_to_global;        /* [M] */
  const float *sigma, *conic, *J, *precomputed_rgb, *radius; /* [M,6] [M,3] [M,6] [M,3] [M,4] */
  const float *uv_selected, *xyz_c_selected;                 /* [M,2] [M,3] */
  const int *sorted_gaussians;         /* [S] compacted ids */
  const int *splat_start_end_idx_by_tile_idx; /* [T+1] */
  const float *image, *weight_per_pixel;      /* [H,W,3] [H,W] */
  const int *splats_per_pixel;                /* [H,W] */
} gsplat_forward_view;

typedef struct gsplat_gradients {      /* GaussianGradients (leaf part), compacted order [M,...], caller-owned */
  /* grad_sh may be NULL (ABI 5): a single-view optimizer can rebuild the SH gradients from grad_precompute_rgb and the
   * viewing direction (gsplat_optimizer_step_sh_factored); the backward then skips their 12 (l_max+1)^2 - 12 bytes. */
  float *grad_xyz, *grad_rgb, *grad_sh, *grad_opacity, *grad_scale, *grad_quaternion;
  /* optional intermediates (may be NULL): */
  float *grad_conic, *grad_uv, *grad_J, *grad_sigma, *grad_xyz_c, *grad_precompute_rgb;
} gsplat_gradients;

/* r06: the optimizer state the per-gaussian backward needs to apply the masked Adam step itself
 * (gsplat_backward_gaussians_adam).  Groups in this order: 0 xyz, 1 rgb (band 0), 2 sh, 3 opacity, 4 scale, 5 quaternion;
 * moments in GLOBAL order next to the parameters, laid out like them (quaternion moments 16-byte aligned); group 2 is
 * ignored when l_max == 0. */
typedef struct gsplat_adam_fused {
  float *exp_avg[6], *exp_avg_sq[6];
  float lr[6];                       /* per group (cuda/trainer.cu:1049-1071) */
  float b1, b2, eps, bias1, bias2;   /* include/gsplat_cuda/optimizer.cuh:9-11; bias_k = 1 - b_k^(iteration + 1) */
  float *uv_grad_accum;              /* [N] += |grad_uv| of the visible gaussians; may be NULL */
  int *grad_accum_dur;               /* [N] += 1 for the visible gaussians; may be NULL */
  int mode;                          /* 0: all six groups in the kernel.  1: band 0, opacity, scale, quaternion and the
                                      * statistics in the kernel; it stores grad_xyz and grad_precompute_rgb (`out` must hold
                                      * them) and the caller runs gsplat_optimizer_step_sh_factored and then
                                      * gsplat_optimizer_step on the xyz group alone -- the positions must not move before
                                      * the SH group has taken its directions from them.  2: all six groups, in TWO kernels:
                                      * the SH group's step in a kernel of its own in front, which reads the coefficient rows
                                      * once -- for the update and for the sums over them that the position gradient needs
                                      * (handed on in a [M,3] array of the context) -- then the per-gaussian backward with the
                                      * five small groups, which no longer reads the SH rows at all.  Same bits as modes 0, 1 */
} gsplat_adam_fused;

int gsplat_context_create(gsplat_context **out, int max_gaussians, int max_width, int max_height);
int gsplat_context_destroy(gsplat_context *ctx);
/* bytes of device memory currently held by the context */
size_t gsplat_context_bytes(const gsplat_context *ctx);

int gsplat_rasterize_image(gsplat_context *ctx, const gsplat_gaussians *gaussians, const gsplat_camera *camera,
                           const gsplat_raster_config *config, float bg_color, int l_max,
                           gsplat_forward_view *out, void *stream);

/* Consumes the state left in ctx by the last gsplat_rasterize_image.  All leaf gradients are
 * overwritten ("=" on a zeroed buffer, i.e. the state after zero_grads + backward_pass). */
int gsplat_backward_pass(gsplat_context *ctx, const gsplat_gaussians *gaussians, const gsplat_camera *camera,
                         const float *grad_image, float bg_color, int l_max, const gsplat_gradients *out,
                         void *stream);
/* r06 -- single-GPU training: gsplat_backward_gaussians and the optimizer step of TrainerImpl::optimizer_step
 * (cuda/trainer.cu:1027-1158) in ONE pass over the visible gaussians.  The kernel differentiates a gaussian and applies
 * adam_kernel's update (cuda/optimizer.cu:6-29: NaN gradient -> 0, bias-corrected moments) to its rows of all six
 * parameter groups IN PLACE -- through the pointers of `gaussians`, which this entry point writes -- and of their moments,
 * the SH group from the factored gradient (gsplat_optimizer_step_sh_factored's product), and adds |grad_uv| / 1 to the
 * densification statistics.  Call it where gsplat_backward_gaussians would be called (after gsplat_backward_render).
 * Parameters, moments and statistics come out bit-identical to gsplat_backward_gaussians (grad_sh NULL) +
 * gsplat_optimizer_step_sh_factored + gsplat_optimizer_step; what is saved is the gradients' round trip through HBM and
 * the second and third read of parameters the backward has just read (~370 of ~2030 bytes per visible gaussian at
 * l_max 3).  `out` may be NULL; when given, its arrays are filled as gsplat_backward_gaussians fills them (except grad_sh,
 * which this form never stores). */
int gsplat_backward_gaussians_adam(gsplat_context *ctx, const gsplat_gaussians *gaussians, const gsplat_camera *cam,
                                   int l_max, const gsplat_adam_fused *opt, const gsplat_gradients *out, void *stream);

/* The same backward in two calls, for hosts that overlap a gradient exchange with it (3dgs_amd/dist.py):
 * gsplat_backward_render runs the compositing backward (render_image_backward) and, if rgb_global != NULL, leaves this
 * view's dL/d(precomputed rgb) in GLOBAL gaussian order in rgb_global[N,3] (zero where culled) -- final at that point,
 * so an all-gather of it can run while gsplat_backward_gaussians executes the per-gaussian operator chain. */
int gsplat_backward_render(gsplat_context *ctx, const float *grad_image, float bg_color, float *rgb_global,
                           void *stream);
int gsplat_backward_gaussians(gsplat_context *ctx, const gsplat_gaussians *gaussians, const gsplat_camera *camera,
                              int l_max, const gsplat_gradients *out, void *stream);
/* The per-gaussian chain for the gaussians with GLOBAL index in [first_gaussian, end_gaussian) only (their compacted
 * slots are contiguous: the compaction keeps the order).  A view-sharded step calls it chunk by chunk and starts the
 * all-reduce of one chunk's twelve common columns (gsplat_pack_gradients_split_range) while the next chunk is computed;
 * the union of the chunks is exactly gsplat_backward_gaussians. */
int gsplat_backward_gaussians_range(gsplat_context *ctx, const gsplat_gaussians *gaussians, const gsplat_camera *camera,
                                    int l_max, const gsplat_gradients *out, int first_gaussian, int end_gaussian,
                                    void *stream);

/* r05 -- the view-sharded step without compacted gradient arrays and without a pack pass (3dgs_amd/dist.py, exchange
 * "split").  What the exchange sums per gaussian is common[N,12] = {grad_xyz 3, grad_opacity, grad_scale 3,
 * grad_quaternion 4, 1.0 if this view saw the gaussian} in GLOBAL gaussian order, plus (training) uv_norm[N] =
 * |grad_uv|; what it gathers is this view's g_rgb[N,3].
 *   gsplat_backward_render_split  = gsplat_backward_render that, in the pass that scatters g_rgb to rgb_global, also
 *                                   clears the rows of `common` / `uv_norm` of the gaussians this view culled;
 *   gsplat_backward_gaussians_split = the per-gaussian operator chain (cuda/trainer.cu:979-1012) whose twelve leaf
 *                                   values go straight into common[compact_to_global[j]] (and |grad_uv| into uv_norm);
 *                                   the SH and band-0 gradients are not stored at all: gsplat_optimizer_step_sh_views
 *                                   rebuilds them from the gathered g_rgb.  [first, end): a range of global indices as in
 *                                   gsplat_backward_gaussians_range.
 * Values are bit-identical to gsplat_backward_gaussians + gsplat_pack_gradients_split (+ gsplat_pack_uv_grad_norm). */
int gsplat_backward_render_split(gsplat_context *ctx, const float *grad_image, float bg_color, float *rgb_global,
                                 float *common, float *uv_norm, void *stream);
int gsplat_backward_gaussians_split(gsplat_context *ctx, const gsplat_gaussians *gaussians, const gsplat_camera *camera,
                                    int l_max, float *common, float *uv_norm, int first_gaussian, int end_gaussian,
                                    void *stream);

/* ABI 9 -- differentiable depth and opacity maps.  With depth mode on, every forward of the context (training, lean and
 * render-only alike) also composites the per-pixel depth in the same pass:
 *   depth(p) = sum_{i < n(p)} alpha_i T_i z_i,   z_i = the camera-space depth of the gaussian (xyz_c.z),
 * i.e. channel 0 of the image render_image would give for the colour (z, 1, 0) over background 0 (not divided by the
 * opacity; the background adds nothing).  The opacity map needs nothing new: alpha(p) = 1 - weight_per_pixel(p).
 *   gsplat_context_set_depth       forwards of this context render depth (0: they do not; the default);
 *   gsplat_context_depth_map       the [H,W] depth of the last forward, valid until the next forward; an error when that
 *                                  forward did not render depth;
 *   gsplat_backward_render_depth   gsplat_backward_render_split with dL/d depth and dL/d alpha ([H,W] each, either may be
 *                                  NULL = zero) next to dL/d image.  Every gradient becomes that of the total: the
 *                                  compositing part (render_image_backward for colour (z, 1, 0), background 0) adds to
 *                                  d/d opacity, conic and uv, and dL/dz = sum_p alpha T dL/d depth reaches grad_xyz (and
 *                                  grad_xyz_c) through the per-gaussian call that follows -- whichever of
 *                                  gsplat_backward_gaussians(_range, _split, _adam) it is.  Both NULL: exactly
 *                                  gsplat_backward_render_split.  Depth or alpha gradients after a forward that did not
 *                                  render depth: GSPLAT_ERR_INVALID_ARG before anything is launched;
 *   gsplat_backward_pass_depth     gsplat_backward_pass with the two extra gradients. */
int gsplat_context_set_depth(gsplat_context *ctx, int enabled);
int gsplat_context_depth_map(gsplat_context *ctx, const float **depth);
int gsplat_backward_render_depth(gsplat_context *ctx, const float *grad_image, const float *grad_depth,
                                 const float *grad_alpha, float bg_color, float *rgb_global, float *common, float *uv_norm,
                                 void *stream);
int gsplat_backward_pass_depth(gsplat_context *ctx, const gsplat_gaussians *gaussians, const gsplat_camera *camera,
                               const float *grad_image, const float *grad_depth, const float *grad_alpha, float bg_color,
                               int l_max, const gsplat_gradients *out, void *stream);

/* Inverse depth and the second moment (no ABI bump: new entry points only).  Two options of depth mode:
 *   inverse   the composited value is s_i = 1/z_i instead of z_i (a v_rcp_f32, 1 ulp; z_i > near_thresh > 0):
 *             depth(p) = sum alpha_i T_i / z_i, what a monocular inverse-depth prior is compared with;
 *   moment    the forward also composites  depth2(p) = Q(p) = sum_{i < n(p)} alpha_i T_i s_i^2  over background 0.  With
 *             A = 1 - weight_per_pixel, D = depth and Q, the distortion loss sum_{j<i} w_i w_j (s_i - s_j)^2 of a pixel is
 *             A Q - D^2 (gsplat_distortion_loss).
 *   gsplat_context_set_depth_mode     switches depth mode on with the options.  gsplat_context_set_depth(ctx, 1) is exactly
 *                                     (0, 0); gsplat_context_set_depth(ctx, 0) clears everything;
 *   gsplat_context_depth_moment_map   the [H,W] Q of the last forward, under gsplat_context_depth_map's rules; an error when
 *                                     that forward ran without the moment option;
 *   gsplat_backward_render_depth2     gsplat_backward_render_depth with grad_depth2 = dL/dQ ([H,W]) after grad_alpha; any of
 *                                     the three maps may be NULL = zero.  dL/dz_i = (sum_p aT dL/dD + 2 s_i sum_p aT dL/dQ)
 *                                     x (inverse ? -s_i^2 : 1) reaches grad_xyz through whichever per-gaussian call
 *                                     follows (_range, _split, _camera and the Adam-inside forms included).  A non-NULL
 *                                     grad_depth2 after a forward without the moment option: GSPLAT_ERR_INVALID_ARG
 *                                     before anything is launched, the caller's arrays untouched.  The moment option has
 *                                     no absgrad form: depth, alpha or moment gradients of a moment forward while
 *                                     gsplat_context_set_absgrad is on are refused the same way;
 *   gsplat_backward_pass_depth2       gsplat_backward_pass_depth with the same extra argument, under the same rules. */
int gsplat_context_set_depth_mode(gsplat_context *ctx, int inverse, int moment);
int gsplat_context_depth_moment_map(gsplat_context *ctx, const float **q);
int gsplat_backward_render_depth2(gsplat_context *ctx, const float *grad_image, const float *grad_depth,
                                  const float *grad_alpha, const float *grad_depth2, float bg_color, float *rgb_global,
                                  float *common, float *uv_norm, void *stream);
int gsplat_backward_pass_depth2(gsplat_context *ctx, const gsplat_gaussians *gaussians, const gsplat_camera *camera,
                                const float *grad_image, const float *grad_depth, const float *grad_alpha,
                                const float *grad_depth2, float bg_color, int l_max, const gsplat_gradients *out,
                                void *stream);

/* Depth regularisers on the maps above (plain grid-stride kernels; every map [rows, cols] float on the device).
 *   gsplat_distortion_loss   A = 1 - T (T = weight_per_pixel).  Per pixel A Q - D^2 and its partials (Q, -2 D, A) are
 *                            evaluated in double from the float maps (formed in float the difference cancels: 5e-5
 *                            absolute on ordinary scenes).  loss = weight x mean over the P = rows x cols pixels;
 *                            grad_alpha (= dL/d(1 - T), what the backward expects), grad_depth, grad_depth2 get
 *                            weight / P x (Q, -2 D, A): overwritten, or added to when `accumulate` is set.  loss_out may be
 *                            NULL; given, it is a device float, overwritten with the sum reduced in double.
 *   gsplat_depth_prior_loss  weight x (1 / P) sum over the pixels with target > 0 of |depth - target|; the other pixels
 *                            add nothing to the loss or the gradient.  grad_depth gets weight / P x sign(depth - target),
 *                            sign(0) = 0 (overwritten, or added to with `accumulate`).  Whether depth and target are z or
 *                            1/z is the caller's business. */
int gsplat_distortion_loss(const float *T, const float *depth, const float *depth2, int rows, int cols, float weight,
                           int accumulate, float *grad_alpha, float *grad_depth, float *grad_depth2, float *loss_out,
                           void *stream);
int gsplat_depth_prior_loss(const float *depth, const float *target, int rows, int cols, float weight, int accumulate,
                            float *grad_depth, float *loss_out, void *stream);

/* Normal maps from the rendered depth, and two losses on them (no ABI bump: new entry points only; gs_normal.hip).  Every
 * map is [rows, cols] (x 3 for a normal, an image or their gradients) float on the device; every pixel is evaluated in
 * double from the float inputs and rounded to float once; every kernel gathers (a thread owns an output pixel, no
 * atomics), so two runs give the same bits.
 *   With A = 1 - T, a pixel is `ok` when A >= alpha_min, depth > 0 and both are finite; its expected depth is
 *   z = depth / A (inverse: A / depth) and its point P = z ((x - cx) / fx, (y - cy) / fy, 1) with x, y the INTEGER pixel
 *   coordinates (where the compositor samples).  At an interior pixel tx = P(x+1,y) - P(x-1,y), ty = P(x,y+1) - P(x,y-1),
 *   c = ty x tx, n = c / |c|: camera coordinates, facing the camera (a fronto-parallel surface: (0,0,-1)).  The normal is
 *   valid when the pixel and its four neighbours are ok and |c| > 0; every other pixel, the one-pixel border included,
 *   gets (0,0,0) exactly -- the "no normal" marker of the losses below.
 *   gsplat_depth_to_normal           writes normal [rows, cols, 3];
 *   gsplat_depth_to_normal_backward  from grad_normal = dL/dn ([rows, cols, 3]) to grad_depth = dL/d depth and grad_alpha =
 *                                    dL/d(1 - T) (what every backward here takes), through n = c / |c|, the cross product,
 *                                    P and z(depth, A).  A pixel's depth enters the normals of its four neighbours only; a
 *                                    pixel no valid normal reads gets 0 exactly.  Either output may be NULL; overwritten,
 *                                    or added to when `accumulate` is set;
 *   gsplat_normal_prior_loss         weight / P x sum over the pixels with a non-zero normal AND a non-zero prior of
 *                                    1 - n . prior / |prior| (P = rows x cols); grad_normal gets -weight / P x prior / |prior|
 *                                    there and 0 elsewhere;
 *   gsplat_normal_smoothness_loss    weight / P x sum over the horizontally or vertically adjacent pairs (a, b) of non-zero
 *                                    normals of w_ab sum_c |n_a,c - n_b,c|, w_ab = exp(-edge_scale x mean_c |I_a,c - I_b,c|)
 *                                    for an image I [rows, cols, 3] (a constant: no gradient), 1 when image is NULL;
 *                                    grad_normal gets the subgradient with sign(0) = 0.
 *   grad_normal of the two losses may be NULL and follows `accumulate`; loss_out may be NULL, given it is a device float
 *   overwritten with the sum reduced in double in a fixed order.  Refused with GSPLAT_ERR_INVALID_ARG before anything is
 *   launched: non-positive sizes, alpha_min outside (0, 1], non-finite intrinsics, fx or fy equal to 0. */
int gsplat_depth_to_normal(const float *depth, const float *T, int rows, int cols, float fx, float fy, float cx, float cy,
                           int inverse, float alpha_min, float *normal, void *stream);
int gsplat_depth_to_normal_backward(const float *depth, const float *T, int rows, int cols, float fx, float fy, float cx,
                                    float cy, int inverse, float alpha_min, const float *grad_normal, int accumulate,
                                    float *grad_depth, float *grad_alpha, void *stream);
int gsplat_normal_prior_loss(const float *normal, const float *prior, int rows, int cols, float weight, int accumulate,
                             float *grad_normal, float *loss_out, void *stream);
int gsplat_normal_smoothness_loss(const float *normal, const float *image, int rows, int cols, float weight,
                                  float edge_scale, int accumulate, float *grad_normal, float *loss_out, void *stream);

/* Camera gradient (no ABI bump: new entry points only).  view (camera->view[0..11] = [R|t]) and campos are two
 * independent inputs, as the forward reads them.  With c_j = dL/d xyz_c of visible gaussian j (projection, screen and
 * depth terms), p_j its world position, dM_j = dL/dM for M = J R and s_j its position gradient through the SH view
 * direction:
 *   grad_view[4r + c] = sum_j c_j[r] p_j[c] + sum_j (J_j^T dM_j)[r][c],  grad_view[4r + 3] = sum_j c_j[r]   (r, c < 3)
 *   grad_campos       = -sum_j s_j
 * summed in double in a fixed order (the same bits in every run) and written as float (device arrays of 12 and 3,
 * overwritten; zeros when nothing is visible).  The intrinsics get no gradient.  A camera whose campos is -R^T t has
 * one pose: 3dgs_amd/pose.py turns the fifteen numbers into its gradient.  The _range, _split and _adam backwards
 * produce no camera gradient.
 *   gsplat_backward_gaussians_camera  gsplat_backward_gaussians that also writes grad_view / grad_campos; its gradient
 *                                     arrays are bit-identical to gsplat_backward_gaussians'.  out may be NULL: then only
 *                                     the camera gradient is produced (pose refinement, localisation).  Needs
 *                                     gsplat_backward_render or gsplat_backward_render_depth since the last forward;
 *   gsplat_backward_pass_camera       gsplat_backward_pass / gsplat_backward_pass_depth (grad_depth, grad_alpha may both
 *                                     be NULL) + the camera gradient. */
int gsplat_backward_gaussians_camera(gsplat_context *ctx, const gsplat_gaussians *gaussians, const gsplat_camera *camera,
                                     int l_max, const gsplat_gradients *out, float *grad_view, float *grad_campos,
                                     void *stream);
int gsplat_backward_pass_camera(gsplat_context *ctx, const gsplat_gaussians *gaussians, const gsplat_camera *camera,
                                const float *grad_image, const float *grad_depth, const float *grad_alpha, float bg_color,
                                int l_max, const gsplat_gradients *out, float *grad_view, float *grad_campos,
                                void *stream);

/* Per-gaussian blend-weight statistics of the last completed forward (no ABI bump: a new entry point only): how much
 * each gaussian contributed to the view, the number contribution-based pruning is built on.  Let visible gaussian j sit
 * at position i of the list of the tile that holds pixel p.  j is composited at p iff i < splats_per_pixel[p] (the
 * forward's own stop index) and its alpha at p passes the forward's 1/255 test; its blend weight there is
 * w_jp = alpha_jp * T_p(before j), with alpha evaluated exactly as the forward evaluates it (0.99 cap included) on the
 * opacity the forward's records carry (anti-aliased compensation and the 3D filter's factor included), and T running the
 * forward's recurrence.  Per gaussian:
 *   weight_sum[j]  sum_p w_jp            accumulated with +=   (float atomics: not bit-reproducible, as the gradient rows)
 *   weight_max[j]  max_p w_jp            accumulated with max  (on the bit pattern, weights are >= 0 and never NaN:
 *                                                               order-independent, bit-reproducible)
 *   pixels[j]      pixels compositing j  accumulated with +=   (int32: bit-reproducible)
 * weight_sum[j] is the pixel sum of the image that would render with colour 1 for j, 0 for every other gaussian and the
 * background; hence sum_j weight_sum[j] = sum_p (1 - weight_per_pixel[p]).  The arrays are device arrays in GLOBAL
 * gaussian order [num_gaussians], accumulated INTO (rows of culled gaussians are not touched): clear them once and call
 * after each view's forward to gather statistics over a camera set.  Any of the three may be NULL, not all of them.
 * num_gaussians must be the recorded forward's.  Works after a training, lean or render-only forward and after a backward
 * of it; refused (GSPLAT_ERR_INVALID_ARG, before any launch) when there is no completed forward: none yet, the last one
 * failed or saw nothing (GSPLAT_ERR_NO_VISIBLE), or its outputs were detached.  `stream` must be the forward's stream or
 * ordered behind it.  A tile list longer than 1488 entries is walked whole by one workgroup. */
int gsplat_context_accumulate_contributions(gsplat_context *ctx, int num_gaussians, float *weight_sum,
                                            float *weight_max, int *pixels, void *stream);

/* Median (quantile) depth of the last completed forward (no ABI bump: a new entry point only): the depth 2DGS, RaDe-GS
 * and gsplat mesh from, where the expected depth sum alpha T z / (1 - T) lies in front of the surface.  For pixel p walk
 * the composited entries of its tile's list front to back as gsplat_context_accumulate_contributions does (entry i is
 * composited iff i < splats_per_pixel[p] and its alpha passes the forward's 1/255 test; alpha capped at 0.99,
 * T <- fma(-alpha, T, T) from T = 1):
 *   index[p]  the list position of the first composited entry whose T AFTER it is <= threshold (float32, on that chain);
 *   depth[p]  the camera-space z of that entry's gaussian, bit for bit as the forward stored it -- always z, never 1/z,
 *             whatever the context's depth mode, and the context need not be in depth mode at all.
 * A pixel whose transmittance never reaches the threshold gets depth 0 and index -1 (every visible gaussian has
 * z > near_thresh > 0: 0 is "no surface here").  threshold must be finite and in (0, 1); 0.5 is the median.  depth and
 * index are [H,W] device arrays of the recorded forward's size, every pixel is written; index may be NULL.  No atomics:
 * the same bits in every run and under either binning route.  For a list the forward walked whole T is the forward's bit
 * for bit, so index[p] >= 0 exactly where weight_per_pixel[p] <= threshold; a segmented forward multiplied its segments'
 * products in another order.  Calling conditions and `stream` as for gsplat_context_accumulate_contributions; refused
 * with GSPLAT_ERR_INVALID_ARG before any launch (the arrays stay as they were): a null context, no recorded forward,
 * another num_gaussians, a threshold outside (0, 1) or not finite, a null or non-device depth, a non-device index.  A
 * tile list longer than 1488 entries is walked whole by one workgroup. */
int gsplat_context_median_depth(gsplat_context *ctx, int num_gaussians, float threshold, float *depth /* [H,W] */,
                                int *index /* [H,W] or NULL */, void *stream);

/* Feature maps of the last completed forward (no ABI bump: new entry points only): the caller's own per-gaussian
 * channels carried through the renderer, and pixel maps lifted back onto the gaussians.  With w_jp the blend weight of
 * gsplat_context_accumulate_contributions above (same entries, same alpha, same T):
 *   gsplat_context_render_features   out[p, c]     = sum_j w_jp features[j, c]        features [N,C], out [H,W,C]
 *   gsplat_context_lift_features     lifted[j, c] += sum_p w_jp map[p, c]             map [H,W,C], lifted [N,C]
 * each the other's adjoint: <render(f), g> = <f, lift(g)> (lifted cleared first).  features and lifted are in GLOBAL
 * gaussian order, 1 <= channels <= 512, all four are dense device arrays.  There is no background term: the map is what
 * the gaussians contribute, the forward's weight_per_pixel says how much of a pixel is left.  render_features writes every
 * pixel of out; a pixel's sum runs in list order without atomics, so the map is bit-reproducible -- in every run, under
 * either binning route, channel by channel at every `channels`, and with the forward's own colours it is the forward's
 * image at background 0.  lift_features ACCUMULATES into lifted (rows of culled gaussians and of gaussians no pixel
 * composited are not touched: clear once, call after each view's forward to gather a camera set) with float atomics: not
 * bit-reproducible in the last bits, as weight_sum.  With a map of ones and channels = 1 it is weight_sum.
 * Neither call differentiates anything: the gradient of a loss on `out` with respect to `features` is lift_features of
 * the loss's gradient map, and its gradient with respect to opacity, conic and position is
 * gsplat_context_features_backward below, which adds it to the gradient rows of the compositing backward.
 * Calling conditions, checks (all before any launch; a refused call leaves the caller's arrays as they were) and `stream`
 * as for gsplat_context_accumulate_contributions; a backward after them is unaffected.  A tile list longer than 1488
 * entries is walked whole by one workgroup (per chunk of 16 channels). */
int gsplat_context_render_features(gsplat_context *ctx, int num_gaussians, int channels,
                                   const float *features /* [N,C], global order */, float *out /* [H,W,C] */,
                                   void *stream);
int gsplat_context_lift_features(gsplat_context *ctx, int num_gaussians, int channels, const float *map /* [H,W,C] */,
                                 float *lifted /* [N,C], global order, += */, void *stream);

/* The feature map's gradient with respect to the GEOMETRY (no ABI bump: a new entry point only).  With grad_map[p, c] =
 * dL/d out[p, c] of a loss on gsplat_context_render_features' map, out is the forward's image with colours `features`,
 * pixel gradient grad_map and background 0, for any number of channels: the call walks the recorded lists back to front
 * as the compositing backward does and ADDS the loss's d/d opacity logit, d/d conic (3) and d/d uv (2) to the gradient
 * rows gsplat_backward_render* left in the context (the 0.99 cap differentiated as if absent, nothing for a gaussian whose
 * sigmoid(opacity) is 1 in float32, as there).  It sits between gsplat_backward_render* of the recorded forward and
 * whichever per-gaussian call follows (gsplat_backward_gaussians, _range, _split, _adam, _camera), which then returns
 * the gradient of the TOTAL loss down to xyz, opacity, scale and quaternion; the anti-aliased mode and the 3D filter
 * need nothing new (their chain sits behind the rows).  Calling it twice adds twice; for a feature loss alone pass a
 * zero grad_image to gsplat_backward_render.  The colour, depth and absgrad columns of the rows are not touched: the
 * absgrad statistic (gsplat_context_set_absgrad) does NOT include the feature term, the signed grad_uv does.  The
 * gradient with respect to `features` stays gsplat_context_lift_features(grad_map).  Float atomics: order-dependent in
 * the last bits, as the rows are.
 * Refused with GSPLAT_ERR_INVALID_ARG, before any launch and with the rows and the caller's arrays untouched: a null
 * context, a null or non-device pointer, channels outside 1..512, num_gaussians not the forward's, no completed forward
 * or its outputs detached (the conditions of gsplat_context_lift_features), and no compositing backward since the last
 * forward.  `stream` must be the backward's stream or ordered behind it.  A tile list longer than 1488 entries is walked
 * whole by one workgroup (per chunk of 16 channels). */
int gsplat_context_features_backward(gsplat_context *ctx, int num_gaussians, int channels,
                                     const float *features /* [N,C], global order */,
                                     const float *grad_map /* [H,W,C] */, void *stream);

/* Training a per-gaussian feature field (no ABI bump: new entry points only; gs_featloss.hip): three losses on a feature
 * map and the feature column's optimizer step.  A map is [rows, cols, channels] float on the device, channel-contiguous
 * as gsplat_context_render_features writes it, 1 <= channels <= 512, P = rows x cols.  As for the depth and normal
 * losses above: every pixel is evaluated in double from the float maps and rounded to float once; grad_map (may be NULL)
 * is overwritten, or added to when `accumulate` is set; loss_out (may be NULL; a device float) is overwritten with the
 * sum reduced in double in a fixed order; no atomics, two runs give the same bits.
 *   gsplat_feature_ce_loss      softmax cross-entropy with the channels as logits and labels int32 [rows, cols]: a pixel
 *                               takes part when 0 <= label < channels;
 *                                 loss = weight / P x sum_p (logsumexp(map[p, :]) - map[p, label_p])
 *                                 grad = weight / P x (softmax(map[p, :]) - onehot(label_p))
 *                               the maximum is subtracted before the (double) exponentials.  Every other label (negative:
 *                               "ignore"; channels or more: out of range) adds nothing to the loss and gets a gradient of
 *                               exactly 0 in every channel;
 *   gsplat_feature_l1_loss      loss = weight / (P channels) x sum |map - target| over the valid pixels, target [rows, cols,
 *                               channels], valid uint8 [rows, cols] (non-zero: valid) or NULL (every pixel);
 *                               grad = weight / (P channels) x sign(map - target), sign(0) = 0, 0 at the other pixels;
 *   gsplat_feature_cosine_loss  loss = weight / P x sum (1 - f.t / (|f||t|)) over the valid pixels with |f| > 0 and |t| > 0
 *                               (f = map[p, :], t = target[p, :]); the gradient goes through the normalisation of f:
 *                               grad = -weight / P x (t - (f.t / |f|^2) f) / (|f||t|); exactly 0 at the other pixels.
 * Refused with GSPLAT_ERR_INVALID_ARG before anything is launched: a non-positive size, channels outside 1..512, a NULL
 * map, labels or target, grad_map and loss_out both NULL.
 *   gsplat_feature_adam_step    gsplat_optimizer_step for one group of stride `channels` whose gradient lies in GLOBAL
 *                               order (where gsplat_context_lift_features adds it): for every j < num_culled the row
 *                               compact_to_global[j] of features, exp_avg and exp_avg_sq ([N, channels]) takes the Adam
 *                               step of gsplat_optimizer_step (the same device function, bit for bit) on the same row of
 *                               grad_global, and that gradient row is then set to zero -- an accumulator that was all
 *                               zero before the view's lift is all zero again (lift_features only touches gaussians the
 *                               forward composited, a subset of the rows the view saw).  Rows the view did not see are
 *                               neither read nor written, in any of the four arrays.  num_culled == 0 launches nothing. */
int gsplat_feature_ce_loss(const float *map, const int *labels /* [rows, cols] */, int rows, int cols, int channels,
                           float weight, int accumulate, float *grad_map, float *loss_out, void *stream);
int gsplat_feature_l1_loss(const float *map, const float *target, const unsigned char *valid /* [rows, cols] or NULL */,
                           int rows, int cols, int channels, float weight, int accumulate, float *grad_map,
                           float *loss_out, void *stream);
int gsplat_feature_cosine_loss(const float *map, const float *target, const unsigned char *valid /* [rows, cols] or NULL */,
                               int rows, int cols, int channels, float weight, int accumulate, float *grad_map,
                               float *loss_out, void *stream);
int gsplat_feature_adam_step(const int *compact_to_global, int num_culled, int channels,
                             float *features, float *exp_avg, float *exp_avg_sq /* [N, channels], global order */,
                             float *grad_global /* [N, channels], global order */, float lr, float b1, float b2,
                             float eps, float bias1, float bias2, void *stream);

/* Per-view appearance compensation with a bilateral grid (no ABI bump: new entry points only; gs_bilagrid.hip;
 * "Bilateral Guided Radiance Field Processing", Wang et al. 2024).  A grid is [12, grid_l, grid_h, grid_w] float on the
 * device, 1 <= grid_w, grid_h <= 64, 1 <= grid_l <= 16; an image is [rows, cols, 3] float.  For pixel (x, y) with colour r:
 *   guidance      g  = 0.299 r0 + 0.587 r1 + 0.114 r2
 *   coordinates   gx = (x + 0.5) / cols x (grid_w - 1), gy = (y + 0.5) / rows x (grid_h - 1),
 *                 gz = clamp(g, 0, 1) x (grid_l - 1)
 *   cell, per axis of n vertices:  i0 = min(floor(c), max(n - 2, 0)), i1 = min(i0 + 1, n - 1), t = c - i0
 *   coefficients  A = the 12 trilinearly interpolated values as a row-major 3x4 matrix (channel = row x 4 + column)
 *   output        out = A[:, :3] r + A[:, 3]
 * which is grid_sample(bilinear, align_corners, border padding) of the grid followed by the affine.  A grid whose
 * channels 0, 5 and 10 are one and the others zero gives the image back; a 1 x 1 x 1 grid is one 3x4 colour affine per view.
 * As for the depth, normal and feature losses: everything is evaluated in double from the float inputs and every stored
 * value is rounded to float once.  Inputs must be finite.
 *   gsplat_bilagrid_slice           out [rows, cols, 3] = the corrected image (out may be image itself).
 *   gsplat_bilagrid_slice_backward  from grad_out = dL/d out: grad_image (or NULL) = dL/d image, WRITTEN, never added to:
 *                                   A[:, :3]^T G plus, through the guidance, (sum_rc G_r dA_rc/dgz [r,1]_c) (grid_l - 1)
 *                                   (0.299, 0.587, 0.114) -- that part is exactly 0 where g <= 0, g >= 1 (the two ends
 *                                   themselves included, as grid_sample's border padding has it) or grid_l == 1;
 *                                   grad_grid (or NULL) [12, grid_l, grid_h, grid_w] = sum over the pixels of
 *                                   wx wy wz G_row [r,1]_col, overwritten, or added to (the once-rounded value) when
 *                                   accumulate_grid is set.  grad_grid is summed in double at every stage WITHOUT atomics:
 *                                   per 32 x 32 pixel tile into a slab of the library's scratch, then per grid value over
 *                                   the tiles in a fixed order -- like out and grad_image it carries the same bits in
 *                                   every run.  The slab is tiles x (vertices a tile touches) x grid_l x 12 doubles.
 *   gsplat_bilagrid_tv_loss         loss = weight x sum over the three axes of (the sum over the adjacent pairs along the
 *                                   axis, all 12 channels, of the squared difference / the number of such pairs); an axis
 *                                   of one vertex adds 0.  grad_grid (or NULL) gets its gradient, overwritten or added to
 *                                   with `accumulate`; loss_out (or NULL; a device float) the loss, summed per block and
 *                                   finished in a fixed order.
 * Refused with GSPLAT_ERR_INVALID_ARG before anything is launched, and before the device is asked anything: a grid size
 * outside the limits, a non-positive image size, a NULL grid, image, out or grad_out, both gradient outputs NULL
 * (grad_grid and loss_out for the TV loss), grad_image overlapping grad_out or image. */
int gsplat_bilagrid_slice(const float *grid, int grid_w, int grid_h, int grid_l, const float *image, int rows, int cols,
                          float *out, void *stream);
int gsplat_bilagrid_slice_backward(const float *grid, int grid_w, int grid_h, int grid_l, const float *image,
                                   const float *grad_out, int rows, int cols, int accumulate_grid,
                                   float *grad_image /* or NULL */, float *grad_grid /* or NULL */, void *stream);
int gsplat_bilagrid_tv_loss(const float *grid, int grid_w, int grid_h, int grid_l, float weight, int accumulate,
                            float *grad_grid, float *loss_out, void *stream);

/* Vector quantisation of row vectors: the k-means behind the compressed scene export's SH codebook (no ABI bump: new
 * entry points only; gs_vq.hip; "Compressed 3D Gaussian Splatting", Niedermayr et al. 2024).  x is [N, D] float, codebook
 * [K, D] float, both on the device, row-major and dense; 1 <= D <= 64, 1 <= K <= 65536, N >= 0 (N = 0: a successful
 * no-op).  Inputs must be finite.
 *   gsplat_vq_assign  index[n] = the centroid k with the smallest score s[n,k] = |c_k|^2 - 2 x_n . c_k, which orders the
 *                     centroids as the squared Euclidean distance does.  The score is a k-ordered float fmaf chain on the
 *                     f32-input matrix cores (|c_k|^2 first, itself a float chain, then the coordinates in order), so a
 *                     centroid whose true distance is within ~1.5e-7 x sum_d (x^2 + c^2 + 2 |x c|) of the nearest one's may
 *                     be returned in its place; exactly equal scores resolve to the LOWEST index.  Every point scans the
 *                     codebook in a fixed order and nothing is added atomically: two runs give the same bits.
 *                     dist (or NULL) [N] = sum_d (x_nd - c_{index[n],d})^2 evaluated in double from the floats and
 *                     rounded to float once -- not the score.
 *   gsplat_vq_update  order [N] lists the rows sorted by (index, row), start [K + 1] the clusters' offsets into it
 *                     (start[0] = 0, start[K] = N).  codebook[k] = the mean of x[order[start[k] .. start[k+1])], summed in
 *                     double by a group of 1 .. 64 lanes per (cluster, coordinate) -- members interleaved over the lanes,
 *                     the lanes combined by a fixed butterfly; the width is a function of N and K alone -- and rounded to
 *                     float once.  An empty cluster keeps its centroid's bits.  No atomics: two runs give the same bits.
 * Refused with GSPLAT_ERR_INVALID_ARG before anything is launched, and before the device is asked anything: D or K outside
 * the limits, a negative N, and (N > 0) a NULL x, codebook, index, order or start. */
int gsplat_vq_assign(const float *x, const float *codebook, int N, int D, int K, int *index, float *dist /* or NULL */,
                     void *stream);
int gsplat_vq_update(const float *x, const int *order, const int *start, int N, int D, int K, float *codebook,
                     void *stream);

/* TSDF fusion of rendered depth maps and mesh extraction (no ABI bump: new entry points only; gs_tsdf.hip; the last step
 * of 2DGS, RaDe-GS and GOF: "A Volumetric Method for Building Complex Models from Range Images", Curless & Levoy 1996).
 * The volume is a dense grid of nodes p(i,j,k) = origin + voxel (i,j,k), 0 <= i < nx and likewise j, k, x fastest in
 * memory, in caller-owned device arrays: tsdf [nz,ny,nx] (meaningful only where weight > 0), weight [nz,ny,nx] (a count
 * of observations), color [nz,ny,nx,3] or NULL.  origin: three HOST floats.  A grid holds at most GSPLAT_TSDF_MAX_NODES
 * nodes (indices of nodes, vertices and faces are 31-bit).  Everything is evaluated in double from the float inputs and
 * rounded to float once; every kernel gathers (one thread per node, x on the lanes), nothing is added atomically, two
 * runs give the same bits.
 *   gsplat_tsdf_integrate  num_views views of one size: depth, T [num_views,rows,cols] and image [num_views,rows,cols,3]
 *                     (NULL exactly when color is) on the device; view [num_views,12] (row-major [R|t]) and intrinsics
 *                     [num_views,4] = (fx, fy, cx, cy), integer pixel coordinates being the sample points, on the HOST.
 *                     For every node and the views in order: x_c = R p + t, z = x_c.z, skip unless z > near;
 *                     u = fx x_c.x / z + cx, v = fy x_c.y / z + cy, the pixel (floor(u + 0.5), floor(v + 0.5)), skip when
 *                     it is outside the image; skip unless the pixel is ok as gsplat_depth_to_normal defines it
 *                     (A = 1 - T >= alpha_min, depth > 0, both finite); d = depth / A (inverse: A / depth), skip when
 *                     max_depth > 0 and d > max_depth; s = d - z, skip when s < -trunc (hidden behind the surface);
 *                     val = min(1, s / trunc) (free space in front of the surface is carved); with the node's weight w:
 *                     tsdf = (w tsdf + val) / (w + 1), color likewise from the pixel's, w = w + 1, capped at max_weight
 *                     when max_weight > 0.  The state is float and rounded once per view, and lives in registers over up
 *                     to gsplat_tsdf_views_per_pass() views: the volume is read and written once per that many views, and
 *                     a batch is bit for bit its views one call at a time.  num_views = 0: a successful no-op.
 *                     Refused with GSPLAT_ERR_INVALID_ARG before anything is launched: a non-positive grid or image size,
 *                     a negative num_views, more than GSPLAT_TSDF_MAX_NODES nodes, voxel or trunc not finite and
 *                     positive, alpha_min outside (0, 1], image without color or the reverse, and (num_views > 0) a NULL
 *                     tsdf, weight, origin, depth, T, view or intrinsics, intrinsics that are not finite, fx or fy 0.
 *   gsplat_tsdf_mark  the counting step of marching tetrahedra on the Freudenthal split: with the corners of a cell
 *                     numbered by bits (x = 1, y = 2, z = 4) its six tetrahedra are {0, a, a|b, 7} for the orderings
 *                     (a, b, c) of the axes; they share the body diagonal and cut every face from its low to its high
 *                     corner, so neighbouring cells agree on their shared face and the surface is closed by construction.
 *                     A node is inside when tsdf < 0 (0 is outside).  A cell is meshed when all eight nodes have
 *                     weight >= min_weight.  Per node n (arrays of the grid's size): cell_ok[n] = the cell whose low
 *                     corner n is is meshed; tri_count[n] = that cell's triangles (0 .. 12); edge_mask[n] bit e = the
 *                     edge of type e from n towards +x, +y, +z, +xy, +xz, +yz, +xyz (e = 0 .. 6) has one end inside and
 *                     belongs to a meshed cell: it carries ONE vertex, shared by every triangle around it;
 *                     vert_count[n] = the number of those bits.
 *   gsplat_tsdf_emit  vert_offset / tri_offset [nodes]: the exclusive prefix sums of vert_count / tri_count, num_vertices
 *                     and num_faces their totals (the caller scans and reads the two totals back).  Vertex order is
 *                     (lower node's linear index, edge type); the vertex of the edge (a, b), a the lower node, is
 *                     p_a + t (p_b - p_a), t = f_a / (f_a - f_b), its colour (vertex_colors, NULL exactly when color is)
 *                     the same interpolation of the nodes' colours.  Face order is (cell's low corner's linear index,
 *                     tetrahedron in the lexicographic order of (a, b, c): xyz, xzy, yxz, yzx, zxy, zyx, then the one or
 *                     two triangles): with the tetrahedron's corners numbered 0..3 = (0, a, a|b, 7), one inside corner i
 *                     and the others (o0, o1, o2) ascending, o1 and o2 swapped when (i, o0, o1, o2) is an odd
 *                     permutation, give the triangle on the edges (i-o0, i-o1, i-o2); one outside corner: the same about
 *                     it with the last two swapped; two inside corners i0 < i1 and the others o0 < o1, swapped when
 *                     (i0, i1, o0, o1) is odd, give q = (i0-o0, i0-o1, i1-o1, i1-o0) as (q0, q1, q2) then (q0, q2, q3);
 *                     for an odd ordering (a, b, c) every triangle's last two indices are swapped.  So
 *                     (v1 - v0) x (v2 - v0) points from inside to outside, along +grad tsdf, towards the cameras.  A
 *                     vertex on a node (t = 0) gives zero-area triangles, which are kept: the topology stays closed.
 *                     Writes outside [0, num_vertices) / [0, num_faces) are dropped, not made.
 * mark and emit are refused with GSPLAT_ERR_INVALID_ARG before anything is launched for a non-positive or too large grid,
 * a NULL required pointer, a NaN min_weight, voxel not finite and positive, totals outside 0 .. 2^31 - 1. */
#define GSPLAT_TSDF_MAX_NODES 2147483647LL
int gsplat_tsdf_integrate(float *tsdf, float *weight, float *color /* or NULL */, int nx, int ny, int nz,
                          const float *origin, float voxel, const float *depth, const float *T,
                          const float *image /* or NULL */, const float *view, const float *intrinsics, int num_views,
                          int rows, int cols, int inverse, float alpha_min, float trunc, float near, float max_depth,
                          float max_weight, void *stream);
/* gsplat_tsdf_integrate for a depth map that already holds the surface (a median depth map of
 * gsplat_context_median_depth, or sensor depth): depth[v,y,x] is the camera-space surface depth d itself.  A pixel is ok
 * when depth is finite and > 0 and either T is NULL (no opacity gate) or 1 - T >= alpha_min.  Everything else -- trunc,
 * carving, max_depth, max_weight, colour, evaluation in double, up to gsplat_tsdf_views_per_pass() views per pass, a batch
 * bit for bit its views one call at a time, the refusals (T excepted) -- is gsplat_tsdf_integrate's: one kernel. */
int gsplat_tsdf_integrate_surface(float *tsdf, float *weight, float *color /* or NULL */, int nx, int ny, int nz,
                                  const float *origin, float voxel, const float *depth, const float *T /* or NULL */,
                                  const float *image /* or NULL */, const float *view, const float *intrinsics,
                                  int num_views, int rows, int cols, float alpha_min, float trunc, float near,
                                  float max_depth, float max_weight, void *stream);
int gsplat_tsdf_views_per_pass(void);
int gsplat_tsdf_mark(const float *tsdf, const float *weight, int nx, int ny, int nz, float min_weight,
                     unsigned char *cell_ok, int *tri_count, unsigned char *edge_mask, int *vert_count, void *stream);
int gsplat_tsdf_emit(const float *tsdf, const float *color /* or NULL */, int nx, int ny, int nz, const float *origin,
                     float voxel, const unsigned char *cell_ok, const unsigned char *edge_mask,
                     const long long *vert_offset, const long long *tri_offset, long long num_vertices,
                     long long num_faces, float *vertices, float *vertex_colors /* or NULL */, int *faces, void *stream);

/* Connected components of an indexed triangle mesh and the gather that drops components (no ABI bump: new entry points
 * only; gs_mesh.hip) -- the cleanup every meshing pipeline ends with (2DGS's post_process_mesh keeps the largest clusters).
 *   gsplat_mesh_components  faces [num_faces,3] int32 into num_vertices vertices, device arrays.  Two vertices are
 *                     connected when a face contains both (connectivity by shared vertices; on a marching-tetrahedra
 *                     mesh it differs from edge adjacency only at non-manifold pinch points).  label[v] = the smallest
 *                     vertex index of v's component (a vertex in no face labels itself); face_count[r] = the number of
 *                     faces of the component whose label is r, 0 at every index that is not a label.  Integers, with
 *                     integer atomics: the same bits in every run whatever the order.  A lock-free union-find (the larger
 *                     root hooked under the smaller by compare-and-swap, paths halved on the way) then a flatten and a
 *                     count launch: the work does not grow with the mesh's diameter; *rounds (host, may be NULL) = the
 *                     number of hook rounds, 1.  A face index outside [0, num_vertices) makes the call fail with
 *                     GSPLAT_ERR_INVALID_ARG: a checking launch and the call's one read-back come first, label and
 *                     face_count are then untouched.  Also refused: negative sizes, a NULL or non-device label or
 *                     face_count (num_vertices > 0) or faces (num_faces > 0).  Synchronises `stream`.
 *   gsplat_mesh_compact  the gather: keep_vertex [num_vertices] (0 / 1), vertex_offset its exclusive prefix sum; a face is
 *                     kept iff its first vertex is (the three vertices of a face share a label, so a selection by
 *                     component is constant over a face), face_offset [num_faces] the exclusive prefix sum of that.  Kept
 *                     vertices, colours (colors and out_colors NULL together) and faces keep their relative order, face
 *                     indices go through vertex_offset.  The outputs hold the kept counts (the caller scans and reads the
 *                     totals back).  No atomics: the same bits in every run. */
int gsplat_mesh_components(const int *faces, int num_faces, int num_vertices, int *label /* [Nv] */,
                           int *face_count /* [Nv] */, int *rounds /* host, may be NULL */, void *stream);
int gsplat_mesh_compact(const float *vertices, const float *colors /* or NULL */, const int *faces, int num_vertices,
                        int num_faces, const unsigned char *keep_vertex /* [Nv] */,
                        const long long *vertex_offset /* [Nv] */, const long long *face_offset /* [Nf] */,
                        float *out_vertices, float *out_colors /* or NULL */, int *out_faces, void *stream);

/* Binning route of the fused forward.  0 (default): automatic -- the LDS counting sort + per-tile depth sort, or, when
 * the previous forward had more than ~768 list entries per tile (dense real scenes) or the tile grid exceeds 16384
 * tiles, stable radix sorts on (depth bits, tile).  1 / 2 force one route.  Both produce identical lists. */
int gsplat_context_set_binning_route(gsplat_context *ctx, int route);

/* Testing / tuning hook for the forward's long-list segments (every value < 0 keeps what is set).
 * poll_budget: how often a segment's workgroup polls for the transmittance published by the workgroups in front of it
 * before it multiplies that product up itself (default 4096; 1 makes every workgroup that is not handed its value at once
 * take that path -- same values, more work).  thin_layer_blocks: layers of fewer segment workgroups run their lists'
 * segments side by side, each publishing its own transmittance product first (default 512; 0: none do, every workgroup
 * waits for the one in front).  gate: the forward splits its long lists when the previous forward's longest chain exceeded
 * gate x the work per resident workgroup (default 3, or GSPLAT_FWD_SEGMENTS_GATE; 0: always).  Results do not depend on
 * any of the three. */
int gsplat_context_set_segment_options(gsplat_context *ctx, int poll_budget, int thin_layer_blocks, float gate);

/* Measurement hook: when enabled, every stage of the two fused passes is bracketed by HIP events on the
 * caller's stream.  Stage ids: 0 project+cull+scan, 1 preprocess+scan, 2 emit + tile sort + ranges + per-tile depth sort, 3 reserved,
 * 4 compositing forward, 5 gradient-row memset, 6 compositing backward, 7 per-gaussian backward.
 * gsplat_context_get_timing synchronises the device, writes the per-stage sum of milliseconds and the number
 * of samples since timing was (re)enabled, and returns the number of stages. */
/* Render-only use (serving): forwards stop writing what only a backward or a training host reads -- Sigma, J, conic,
 * the evaluated SH colour (those four pointers of gsplat_forward_view come back NULL) and the compositing kernels'
 * block masks -- and the backward entry points answer "no forward pass recorded" until it is switched off again.
 * Image, per-pixel counts / transmittance and the sorted lists are unchanged. */
/* r05 -- zero-copy hand-over of a forward's outputs.  The thirteen arrays of the reference's ForwardPassData
 * (cuda_data.cuh:70-86: mask, uv, xyz_c, sigma, conic, J, precomputed_rgb, radius, sorted_gaussians,
 * splat_start_end_idx_by_tile_idx, image, weight_per_pixel, splats_per_pixel -- the pointers the last gsplat_forward_view
 * reported) are blocks of the library's pool; after this call the CALLER owns them and returns each with
 * gsplat_pool_free, and the context takes fresh blocks of the same sizes from the pool at its next forward (which finds
 * the ones the caller has returned in the meantime: no allocator call in the steady state of a training loop).  The
 * rasterize_image shim (include/gsplat_cuda/raster.cuh) uses it instead of thirteen device-to-device copies.  The
 * context's fused backward is unavailable for that forward afterwards (the stand-alone operators take the arrays). */
int gsplat_context_detach_forward_outputs(gsplat_context *ctx);
/* The compaction the last completed forward of `ctx` already computed for its cull mask: *mask = the mask array that
 * forward wrote (the pointer gsplat_forward_view reported, whoever owns the block now), *slots[i] = compacted slot of
 * gaussian i where mask[i] is set (its exclusive scan; the entries of culled gaussians are unspecified),
 * *compact_to_global[j] = gaussian of slot j, for N = *num_gaussians and M = *num_culled.  All of it is valid until the
 * context's NEXT forward and describes the mask's contents as that forward wrote them.  NULL pointers when there is none.
 * The drop-in compact_masked_array uses it when it is handed that very mask array (cuda/trainer.cu:941-964, 1028-1044:
 * the host compacts ~25 arrays per iteration by pass_data.d_mask): gsplat_compact_rows_ranked then needs one launch and
 * no scan of the mask. */
int gsplat_context_last_compaction(gsplat_context *ctx, const unsigned char **mask, const int **slots,
                                   const int **compact_to_global, int *num_gaussians, int *num_culled);
/* compact_masked_array with the slots given: dst[slots[i], :] <- src[i, :] for every i with mask[i] set and
 * slots[i] < dst_rows.  One launch. */
int gsplat_compact_rows_ranked(const float *src, const unsigned char *mask, const int *slots, int N, int stride,
                               float *dst, int dst_rows, void *stream);
/* dst[0..n) <- value on `stream`, asynchronously (hipMemsetAsync for 0.0f).  What the drop-in headers route the host's
 * thrust::fill_n calls on float device vectors to (cuda_data.cuh: zero_grads' twelve fills, cuda/trainer.cu:247-261, each
 * of which otherwise ends in a stream synchronisation inside thrust). */
int gsplat_fill_f32(float *dst, size_t n, float value, void *stream);
/* rows[j] <- index of the j-th set entry of mask[0..N) for j < rows_cap (the row list of a compaction; what the lazy
 * SH compaction of the drop-in headers gathers through).  No read-back. */
int gsplat_mask_selected_rows(const unsigned char *mask, int N, int *rows, int rows_cap, void *stream);
int gsplat_context_set_render_only(gsplat_context *ctx, int enabled);
/* Lean forward (training through the fused entry points): gsplat_backward_pass recomputes Sigma, J and the conic from
 * the parameters and never reads the evaluated SH colour, so a caller that does not look at those four arrays of
 * ForwardPassData (cuda_data.cuh:70-86) can switch their stores off: the four pointers of gsplat_forward_view come back
 * NULL, and so do the uncompacted `uv` / `xyz_c` (the compacted uv_selected / xyz_c_selected stay); the per-gaussian
 * forward then writes 104 instead of 176 bytes per visible gaussian and the cull 5 instead of 25 per gaussian.  Image, lists, radii and all
 * gradients are unchanged.  Off by default: the reference's own backward_pass (cuda/trainer.cu:941-1012) hands these
 * arrays to the stand-alone backward operators. */
int gsplat_context_set_lean_forward(gsplat_context *ctx, int enabled);
/* r06: how the per-gaussian forward is launched (GSPLAT_PRE_SPLIT in the environment sets the default of new contexts).
 * 0 (default): the single fused kernel.  1: two kernels one behind the other on `stream` -- the SH colour as a stream
 * of its own (SH rows through LDS as linear spans), then geometry / record / tile count with the colour read back.
 * 2: the same two kernels side by side -- the colour kernel on a low-priority stream of the context, forked behind the
 * cull and joined in front of the binning kernels; it writes the colour straight into the 48-byte records.  The reference
 * launches compute_rgb_from_sh and the covariance chain separately too (cuda/raster.cu:78-100).  Every output is
 * bit-identical in all modes; on MI355X modes 1 and 2 measure 25 and 40 us SLOWER than mode 0 at 1e6 gaussians
 * (profiles/r06_ab_preprocess_split.txt) -- they are kept as the measured answer to "split it", not as a recommendation. */
int gsplat_context_set_preprocess_split(gsplat_context *ctx, int mode);
/* What the forwards of this context did so far: out[0] forwards completed, out[1] forwards whose speculatively queued
 * tail (placement, per-tile sorts, compositing: queued before the host has seen the counts, from the previous forward's
 * figures) had to be redone because the instances outgrew the buffers or the longest list needed a sort kernel that
 * was not queued, out[2] forwards that walked the compacted slots, out[3] growths of the instance buffers, out[4]
 * compositing backwards that took their tiles heaviest first (scenes whose longest tile list was more than three times
 * the average in the forward before), out[5] compositing backwards that walked lists of more than 1488 entries as
 * segments of 496 with a workgroup each (the forward before had such a list; the forward stores a per-pixel checkpoint
 * at every segment boundary it reaches), out[6] forwards in which every segment of such a list was a workgroup of its
 * own (r06: counted once per forward, a redone tail included), out[7] / out[8] the largest stop index of any tile and the
 * sum of the tiles' largest stop indices in the last forward that published them (contexts that have seen a list beyond
 * 1488 entries).  The forward splits when the figures of the forward TWO back say max * 2048 > 3 * sum: those are the
 * newest ones the host knows to be complete without synchronising, so the decision -- and with it the bits of the image
 * -- never follows host / GPU timing (r06).  out[9] segment workgroups of split forwards whose polls for the workgroup
 * in front ran out and which multiplied the transmittance product up themselves (results identical; every one of them
 * is work done twice).  out[10] compositing backwards that walked compact lists (gsplat_context_set_compact_lists), out[11]
 * the useful entries of the last forward's tile lists -- the sum over the tiles of what their workgroups ranked; 0 when
 * that forward wrote no compact lists; asked for (n > 11), it waits for the device and copies one int per tile.  out[12]
 * per-gaussian backwards that read the forward's SH direction sums (gsplat_context_set_dir_sums), out[13] per-gaussian
 * backwards that read the SH rows instead (every other form, and every backward whose forward left no sums it may use).
 * Writes min(n, 14) values and returns 14. */
int gsplat_context_get_counters(gsplat_context *ctx, long long *out, int n);
/* Compact lists for the compositing backward (new entry point, no signature changed; default on).  A tile list holds
 * every gaussian whose mh_dist box touches the tile; about a quarter of the entries reach no 4x4 pixel block of the tile
 * with alpha >= 1/255 and contribute nothing to the image or to any gradient.  With the switch on, the compositing forward
 * of a training context also writes, per tile, the entries that can contribute, in list order, and per pixel the stop
 * index counted in those; gsplat_backward_render* then walks only them.  Image, transmittance, stop indices and the lists
 * of gsplat_forward_view are the same bits either way; gradients are the same sums with fewer zero terms (the order of the
 * float atomics differs, as it does between any two runs).  Read by the next gsplat_rasterize_image; a backward follows
 * its forward.  The full lists are used instead, silently, where compact ones are not written: render-only contexts, the
 * radix binning route, and contexts whose last forward had a list beyond 1488 entries (the segment paths; a forward whose
 * own longest list exceeds that hands over its full lists too).  GSPLAT_NO_COMPACT_LISTS=1 in the environment forces the
 * switch off. */
int gsplat_context_set_compact_lists(gsplat_context *ctx, int enabled);
/* The SH direction sums (new entry point, no signature changed; default on).  The per-gaussian backward needs the SH
 * coefficient rows for one thing only: nine sums over the row, sum_k dY_k/d(axis) * coefficient[k][channel], from which the
 * position gradient through the view direction is made (the coefficient gradients g_rgb[c] * Y_k need no coefficient).  With
 * the switch on, the fused per-gaussian forward (SH degree 1 and up) of a context that is not render-only forms those sums while the row is in
 * its registers for the colour and stores them (36 bytes per visible gaussian); gsplat_backward_gaussians / _range / _split
 * and gsplat_backward_pass* in their plain form, and gsplat_backward_gaussians_adam with mode 1, then read the sums instead
 * of the row, band 0 and the camera-space position (204 bytes).  The sums are the backward's own, formed by the same code in the same order on the same inputs: every output
 * of the forward and every gradient is bit for bit what it is with the switch off.  A backward reads the sums only of the
 * forward it differentiates, at that forward's degree, given the parameter arrays and camera centre that forward was given;
 * forwards that do not write them (two-kernel forms, anti-aliased mode, render-only contexts) leave none, an Adam backward
 * (which steps parameters in place) leaves them nobody's, and the Adam modes 0 and 2, the camera and the anti-aliased forms
 * of the backward never read them: all of those read the rows, as before.  The sums cost the forward about 10 us per 1e6
 * gaussians at degree 3: a context whose backwards are all of a form that does not read them should switch them off (the
 * Trainer does, from its Adam mode).  "Given the arrays" is a comparison of POINTERS: a caller that rewrites xyz, rgb, sh or
 * the view matrix in place between a forward and its backward gets the forward's sums and a camera-space position
 * recomputed from the arrays as they then are, where the path that reads the rows takes the rows as they then are and the
 * position the forward stored -- neither is the gradient of that forward; do not do that.  Read by the next
 * gsplat_rasterize_image (whether it writes the sums) and by every per-gaussian backward (whether it may read them).
 * GSPLAT_NO_DIR_SUMS=1 in the environment forces the switch off, whatever is set.  gsplat_context_get_counters out[12] /
 * out[13] count the backwards of either kind. */
int gsplat_context_set_dir_sums(gsplat_context *ctx, int enabled);
int gsplat_context_set_timing(gsplat_context *ctx, int enabled);
/* The same for a subset of the stages (bit k of stage_mask = stage k; 0 switches timing off).  Every timed stage
 * costs two event records per call, about 0.7 % of a 1 ms step each: bench.py times only stage 6 inside its timed
 * region and all stages in a separate pass. */
int gsplat_context_set_timing_stages(gsplat_context *ctx, unsigned int stage_mask);
int gsplat_context_get_timing(gsplat_context *ctx, double *stage_ms_sum, long long *stage_count, int max_stages);

/* View-sharded training support: scatter compacted per-view gradients into one global-order
 * row-major buffer packed[N, 12 + 3*n_coeffs] = [xyz3 | band0 3 | sh 3(n_coeffs-1) | opacity1 | scale3 | quat4 |
 * visible1], zero where culled, ready for one RCCL all-reduce. */
int gsplat_pack_gradients_global(gsplat_context *ctx, const gsplat_gradients *grads, int l_max, int num_gaussians,
                                 float *packed, void *stream);
int gsplat_packed_gradient_width(int l_max);

/* Smaller exchange payload for the same result.  Every SH-coefficient gradient of one view is g_rgb[3] x Y_k(dir),
 * so a rank only has to ship g_rgb: factored[N, 12 + 3*world] = [xyz3 | opacity1 | scale3 | quat4 | visible1 |
 * g_rgb of rank 0 | ... | g_rgb of rank world-1] (a rank fills only its own slot; the SUM all-reduce gathers the
 * slots).  gsplat_unpack_gradients_factored rebuilds the global-order packed[N, 12+3*n_coeffs] buffer from the
 * reduced rows, the gaussian positions and all ranks' camera positions campos_all[world,3] (device pointer).
 * gsplat_backward_pass must have been given grad_precompute_rgb. */
int gsplat_factored_gradient_width(int world_size);
int gsplat_pack_gradients_factored(gsplat_context *ctx, const gsplat_gradients *grads, int num_gaussians, int rank,
                                   int world_size, float *factored, void *stream);
int gsplat_unpack_gradients_factored(const float *xyz, const float *campos_all, const float *factored, int l_max,
                                     int num_gaussians, int world_size, float *packed, void *stream);


/* The same factorisation as two collectives with less traffic: common[N,12] = [xyz3 | opacity1 | scale3 | quat4 |
 * visible1] is SUM all-reduced, and every rank's g_rgb[N,3] (+ its camera position in row N) is all-gathered into
 * rgb_all = world blocks of rank_stride floats (block r = rank r's [N,3] g_rgb followed by campos[3]).  At 8 ranks
 * and SH degree 3 a rank moves 2*(7/8)*48 MB + 7*12 MB = 168 MB per step instead of 252 MB (one factored all-reduce)
 * or 420 MB (full rows).  rgb may be NULL when gsplat_backward_render already produced it.  The unpack may be issued in
 * two halves that write disjoint columns of `packed`: common == NULL rebuilds only the SH columns (it can run while the
 * all-reduce of `common` is still in flight), rgb_all == NULL places only the twelve reduced columns. */
int gsplat_pack_gradients_split(gsplat_context *ctx, const gsplat_gradients *grads, int num_gaussians, float *common,
                                float *rgb, void *stream);
/* Rows [first_gaussian, end_gaussian) of `common` (and of `rgb` when given) only: the chunked exchange. */
int gsplat_pack_gradients_split_range(gsplat_context *ctx, const gsplat_gradients *grads, int num_gaussians,
                                      int first_gaussian, int end_gaussian, float *common, float *rgb, void *stream);
int gsplat_unpack_gradients_split(const float *xyz, const float *common, const float *rgb_all, size_t rank_stride,
                                  int l_max, int num_gaussians, int world_size, float *packed, void *stream);

/* The per-view densification statistic in global gaussian order: uv_norm[i] = |grad_uv| of this view's backward
 * (PositionalGradientNorm, cuda/trainer.cu:1143-1148) or 0 where the view culled the gaussian.  SUM all-reduced next
 * to the gradients it feeds gsplat_optimizer_step_packed, so that density control runs on a view-sharded step.
 * grads->grad_uv must have been requested from the backward. */
int gsplat_pack_uv_grad_norm(gsplat_context *ctx, const gsplat_gradients *grads, int num_gaussians, float *uv_norm,
                             void *stream);

/* Absolute screen-space gradients ("absgrad") for densification.  grad_uv[j] is the SIGNED sum over the pixels p that
 * composite gaussian j of the pixel's share (du_p, dv_p) of dL/d uv (render_image_backward adds exactly these, the
 * 0.5 W / 0.5 H factors and, with depth gradients, the depth and alpha terms included); on a large blurry splat the
 * shares of opposite sides cancel and |grad_uv| never reaches the threshold.  In absgrad mode the compositing backward
 * also forms
 *   abs_uv[j] = ( sum_p |du_p| , sum_p |dv_p| ),      absnorm[j] = sqrtf(abs_u^2 + abs_v^2)  >=  |grad_uv[j]|,
 * and every densification statistic the library writes -- uv_norm of gsplat_backward_render_split /
 * gsplat_backward_gaussians_split, uv_grad_accum of gsplat_backward_gaussians_adam (modes 0, 1, 2) -- is absnorm instead
 * of |grad_uv|.  grad_uv itself and every gradient array are what they are with the mode off.
 *   gsplat_context_set_absgrad  a mode of the context (default 0), read by the next gsplat_backward_render* call; it asks
 *                               nothing of the forward: training, lean and depth forwards alike;
 *   gsplat_context_absgrad_uv   abs_uv[M,2] (compacted order, 8-byte aligned) of the last compositing backward.
 *                               GSPLAT_ERR_INVALID_ARG before anything is launched when that backward did not run in
 *                               absgrad mode, when there has been none since the last forward, or when the context is
 *                               render-only;
 *   gsplat_pack_absgrad_norm    uv_norm[N] = absnorm in global gaussian order, 0 where the view culled the gaussian: what
 *                               gsplat_pack_uv_grad_norm is to |grad_uv|, for hosts that keep the unfused path.  The same
 *                               refusals.
 * The sums live in the context's gradient rows: they are valid from the compositing backward until the next forward of
 * the context (which clears the rows), whichever per-gaussian calls run in between. */
int gsplat_context_set_absgrad(gsplat_context *ctx, int enabled);
int gsplat_context_absgrad_uv(gsplat_context *ctx, float *abs_uv, void *stream);
int gsplat_pack_absgrad_norm(gsplat_context *ctx, int num_gaussians, float *uv_norm, void *stream);

/* Anti-aliased rasterization: opacity compensation for the 0.3 px blur (Mip-Splatting; gsplat's
 * rasterize_mode="antialiased").  Every projected covariance gets +0.3 on its diagonal, which dilates a sub-pixel splat
 * without dimming it.  With a, b, c the entries of M Sigma M^T before the blur, a' = a + 0.3f, c' = c + 0.3f,
 *   det0 = a c - b^2,   det1 = a' c' - b^2,   rho = sqrtf(fmaxf(0, det0 / det1))      (a NaN or negative ratio gives 0)
 * and in the mode a gaussian composites with the effective opacity o = sigmoid(logit) * rho.  Conic, radii, culling and
 * tile lists are unchanged; a gaussian with rho == 0 contributes nothing and receives zero gradient.  The backward: the
 * compositing backward's opacity gradient is g_eff = dL/d logit(o); the per-gaussian backward forms
 *   k = g_eff / (1 - o) (0 where 1 - o == 0),   dL/d logit = k (1 - sigma),   dL/d rho = k / rho (0 where rho == 0),
 * and dL/d rho reaches J, Sigma and the position through d rho/d det0 = 1 / (2 rho det1), d rho/d det1 = -rho / (2 det1),
 * d det0/d(a, b, c) = (c, -2b, a), d det1/d(a, b, c) = (c', -2b, a').  There is no gradient through the clamp.
 *   gsplat_context_set_antialiased  a mode of the context (default 0), read by the next gsplat_rasterize_image; a backward
 *                                   follows the mode its forward ran in.  Lean, full, depth and absgrad contexts alike; rho
 *                                   is recomputed by the backward, nothing is stored.
 * With the mode on, GSPLAT_ERR_INVALID_ARG before anything is launched from: gsplat_rasterize_image when the two-kernel
 * forward is selected (gsplat_context_set_preprocess_split != 0); gsplat_backward_gaussians_adam (it steps the opacity
 * before the covariance chain exists); gsplat_backward_gaussians_camera / gsplat_backward_pass_camera.
 * The two operators below are the new arithmetic by itself (one thread per gaussian, gsplat_compute_conic's shape):
 *   gsplat_compute_conic_antialiased            gsplat_compute_conic plus compensation[N] = rho;
 *   gsplat_compute_conic_antialiased_backward   gsplat_compute_conic_backward plus compensation_grad[N] = dL/d rho:
 *                                               J_grad_in +=, sigma_grad_in += of both terms. */
int gsplat_context_set_antialiased(gsplat_context *ctx, int enabled);
int gsplat_compute_conic_antialiased(const float *xyz, const float *view, const float *sigma, float focal_x,
                                     float focal_y, float tan_fovx, float tan_fovy, float mh_dist, int N, float *J,
                                     float *conic, float *radius, float *compensation, void *stream);
int gsplat_compute_conic_antialiased_backward(const float *J, const float *sigma, const float *view, const float *conic,
                                              const float *conic_grad_out, const float *compensation_grad_out, int N,
                                              float *J_grad_in, float *sigma_grad_in, void *stream);

/* 3D smoothing filter (no ABI bump: new entry points only): the other half of Mip-Splatting.  Every gaussian is
 * band-limited to the sampling rate of the training cameras that see it.  For gaussian i and camera k (view [R|t], proj,
 * focal_x, width W, height H), with (x, y, z) the camera-space position and (u, v) the pixel coordinates the forward
 * computes, camera k SAMPLES i when z > near, -0.15 W <= u <= 1.15 W and -0.15 H <= v <= 1.15 H;
 *   t_i = min over the sampling cameras of z / focal_x_k   (no camera samples i: the maximum of t over the sampled
 *         gaussians, 0 when there is none),        filter3d[i] = sqrtf(0.2f) t_i.
 * The filter is constant with respect to the camera a view is rendered from: with s_k = exp(scale_k), f = filter3d[i] and
 * sigma = sigmoid(opacity) a gaussian enters the rasterizer with
 *   scale_eff_k = 1/2 log(s_k^2 + f^2)              (Sigma_eff = Sigma + f^2 I, R being orthonormal),
 *   rho3        = sqrt(prod s_k^2 / prod (s_k^2 + f^2)) = exp(sum_k (scale_k - scale_eff_k)),
 *   opacity_eff = logit(o),  o = sigma rho3,
 * and with w_k = s_k^2 / (s_k^2 + f^2), g_s / g_o the gradients with respect to the effective values and
 * q = g_o / (1 - o) (0 where 1 - o == 0 in float):
 *   grad_scale_k = g_s_k w_k + q (1 - w_k),        grad_opacity = q (1 - sigma).
 * A row with f == 0 passes through both ways with its bits unchanged.
 *   gsplat_compute_filter3d         views / projs [V,16] row-major, focal_x [V], sizes [V,2] = (width, height) ints, all
 *                                   device arrays; near >= 0 (Mip-Splatting: 0.2) -> filter3d [N].  One thread per
 *                                   gaussian walks all V cameras; no host read-back; the same bits in every run;
 *   gsplat_filter3d_apply           (scale [N,3], opacity [N], filter3d [N]) -> scale_eff [N,3], opacity_eff [N];
 *   gsplat_filter3d_apply_backward  the chain rule, IN PLACE on stored gradients: gradient row j (j < M) belongs to
 *                                   gaussian rows[j] (rows == NULL: j) and lies at grad_scale + j * scale_stride (three
 *                                   floats) and grad_opacity + j * opacity_stride, strides in floats: [M,3] / [M] arrays
 *                                   of gsplat_gradients (3, 1) and columns 4..6 / 3 of twelve-float rows (12, 12) alike;
 *   gsplat_context_set_filter3d     filter3d [N] in global order, device memory, caller-owned and valid until it is
 *                                   replaced; NULL (the default) switches the mode off.  Read by the next
 *                                   gsplat_rasterize_image; a backward follows the forward it belongs to.  The forward
 *                                   first writes scale_eff / opacity_eff into two arrays of the workspace (allocated by the
 *                                   first forward in the mode) and then runs, unchanged, on them: conic, radii, culling and
 *                                   tile lists are those of the filtered gaussians, and in anti-aliased mode the
 *                                   compositing opacity is sigma rho3 rho with rho of the filtered covariance.  Every
 *                                   per-gaussian backward that recomputes from parameters (gsplat_backward_pass, _depth,
 *                                   _camera, gsplat_backward_gaussians, _range, _camera, _split) reads the same two arrays
 *                                   and then applies the chain rule to the scale and opacity gradients it has written
 *                                   (when both were requested; _range: its slots; _split: the visible rows of `common` in
 *                                   its range), so `gaussians` and the gradients are those of the RAW parameters.  The
 *                                   camera gradient is that of the filtered image.  gsplat_backward_gaussians_adam (all
 *                                   modes): GSPLAT_ERR_INVALID_ARG before anything is launched -- it would step the
 *                                   parameters it differentiates, and those are the effective ones.
 * The stand-alone operators are untouched: a host that drives them calls the two apply operators around them. */
int gsplat_compute_filter3d(const float *xyz, int N, const float *views, const float *projs, const float *focal_x,
                            const int *sizes, int V, float near_thresh, float *filter3d, void *stream);
int gsplat_filter3d_apply(const float *scale, const float *opacity, const float *filter3d, int N, float *scale_eff,
                          float *opacity_eff, void *stream);
int gsplat_filter3d_apply_backward(const float *scale, const float *opacity, const float *filter3d, const int *rows,
                                   int M, float *grad_scale, int scale_stride, float *grad_opacity, int opacity_stride,
                                   void *stream);
int gsplat_context_set_filter3d(gsplat_context *ctx, const float *filter3d);

#ifdef __cplusplus
}
#endif
#endif /* GSPLAT_HIP_H */
