// gs_context.h -- struct gsplat_context: the persistent workspace of the device-resident per-view pass, the state of its
// last forward, and the process-wide environment switches its users read.  INTERNAL: only the files that implement
// gsplat_* functions taking a context include it (gs_context.hip: life cycle, setters, counters, timing; gs_fused.hip: the
// forward and backward host paths; gs_exchange.hip: the multi-GPU exchange's entry points).  Kernel files do not: what a
// launcher needs of the context reaches it as plain pointers and numbers (gs_pergaussian_args.h).
#pragma once
#include "gs_common.h"
#include "gs_render.h"

namespace gs {

// ---- environment switches, each read once per process (gs_context.hip) ----
// GSPLAT_PRE_SPLIT=0|1|2: the per-gaussian forward as one kernel (the default), as sh_colour_kernel + preprocess_geom_kernel
// one behind the other, or side by side on two streams (r06: built, bit-identical, measured slower -- see sh_colour_kernel,
// gs_preprocess.hip); per context: gsplat_context_set_preprocess_split
int pre_split_default();
// GSPLAT_PRE_JOIN=late: the caller's stream waits for the colour kernel only in front of render_fwd (the first reader of
// the records' colour), not in front of the binning kernels
bool pre_join_late();
// GSPLAT_NO_TILE_ORDER=1: the backward takes its tiles in the plain XCD-run order (A/B of r04's heaviest-first order)
bool no_tile_order();
// GSPLAT_NO_COMPACT_LISTS=1: the backward walks the full tile lists whatever the context's switch says (A/B of the compact
// lists; gs_render.h: CompactLists)
bool no_compact_lists();
// GSPLAT_NO_SEGMENTS=1: long lists stay whole in the backward (A/B of r05's segment split)
bool no_segments();
// GSPLAT_NO_FWD_SEGMENTS=1: one block per tile in the forward, whatever the list lengths (A/B)
bool no_fwd_segments();
// GSPLAT_FWD_SEGMENTS_GATE=<x>: the forward splits its long lists when the longest chain exceeds x times the work per
// resident workgroup (default 3; 0: always)
double fwd_segments_gate();
// GSPLAT_NO_DIR_SUMS=1: no forward writes and no backward reads the SH direction sums, whatever the context's switch says
// (A/B, as GSPLAT_NO_COMPACT_LISTS; gsplat_context_set_dir_sums)
bool no_dir_sums();

}  // namespace gs

struct gsplat_context {
  int max_gaussians = 0, max_width = 0, max_height = 0;
  // per-gaussian, global order
  gs::DeviceBuffer mask, counters, rank, xyz_c_all, uv_all;
  // per-gaussian, compacted order
  gs::DeviceBuffer c2g, xyz_c, uv, sigma, conic, J, rgb, radius, recs, counts, offsets, grad_rows, hitmask;
  // instances
  gs::DeviceBuffer keys_a, keys_b, pay_a, pay_b, sorted, temp, bin_table;
  gs::DeviceBuffer blockmasks;  // per instance: the 16 block bits of the compositing kernels (forward -> backward)
  // per tile / pixel
  gs::DeviceBuffer ranges, image, T_px, n_px;
  // r04: the backward's tiles heaviest first (tile_order_kernel): per tile the largest stop index of its pixels, written
  // by render_fwd, and the order table made from it right behind the forward (off the backward's critical path)
  gs::DeviceBuffer tile_tops, tile_order;
  bool order_ready = false;  // tile_order belongs to the recorded forward
  // Compact lists for the backward (gs_render.h: CompactLists; gsplat_context_set_compact_lists): per instance the useful
  // entries of every tile list and their block masks, per pixel the stop index counted in useful entries, per tile the
  // useful entries its workgroup ranked.  ids_c and masks_c are instance buffers (reserve_instances, instance_room).
  gs::DeviceBuffer ids_c, masks_c, n_c_px, tile_useful;
  bool compact_lists = true;     // the switch; read by the next forward
  bool compact_written = false;  // the last render_fwd launch wrote the compact arrays
  bool compact_ready = false;    // ... and the recorded forward's backwards walk them
  long long n_compact_backwards = 0;
  // r05: long lists split into segments for the backward (gs_render.h: TileSegments); allocated by the first forward that
  // follows one with a list beyond kSegSplitMin
  gs::DeviceBuffer seg_first, seg_extra, seg_chk;
  // ... and for the forward (gs_render.h: FwdSegments)
  gs::DeviceBuffer fseg_first, fseg_blocks, fseg_gran, fseg_part, fseg_stop;
  // depth mode (gsplat_context_set_depth; gs_render.h: DepthMaps): the depth map and the side arrays of the long lists
  bool depth = false;
  bool depth_ready = false;  // the recorded forward rendered depth_map
  bool rows_depth = false;   // the gradient rows carry dL/dz in slot 9 (gsplat_backward_render_depth with depth gradients)
  gs::DeviceBuffer depth_map, seg_chk_d, fseg_part_d;
  // the mode's options (gsplat_context_set_depth_mode; gs_render.h: DepthMaps): s = 1/z, and the second moment Q with its
  // side arrays.  The *_ready pair: what the recorded forward ran with (its backwards follow it, whatever is set by then)
  bool depth_inverse = false, depth_moment = false;
  bool depth_inverse_ready = false, depth_moment_ready = false;
  gs::DeviceBuffer depth2_map, seg_chk_q, fseg_part_q;
  // absgrad mode (gsplat_context_set_absgrad): the compositing backward also sums every pixel's share of dL/d uv by absolute
  // value, into row slots 10 and 11 (gs_render.h: row_moments9r_abs); the densification statistics are made of those
  bool absgrad = false;
  bool rows_abs = false;  // the gradient rows carry those sums (the last compositing backward ran in absgrad mode)
  // anti-aliased mode (gsplat_context_set_antialiased): the forward's records carry sigmoid(logit) * rho, rho the opacity
  // compensation for the 0.3 px blur (gs_math.h: conic_radius<true>); the per-gaussian backward of that forward turns
  // row slot 3 into dL/d logit and the covariance term of dL/d rho
  bool antialiased = false;
  bool fwd_antialiased = false;  // the recorded forward ran in the mode (its backwards follow it, whatever is set by then)
  // 3D smoothing filter (gsplat_context_set_filter3d; gs_filter3d.hip): the forward runs on scale_eff / opacity_eff, which
  // it writes into f3d_scale [max_gaussians,3] / f3d_opacity [max_gaussians] first (allocated by the first forward in the
  // mode); the per-gaussian backwards of that forward recompute from the same two arrays and then apply the chain rule to
  // the scale and opacity gradients they have stored
  const float *filter3d = nullptr;      // caller-owned [N], global order; read by the next forward
  const float *fwd_filter3d = nullptr;  // what the recorded forward ran with (its backwards follow it)
  gs::DeviceBuffer f3d_scale, f3d_opacity;
  void *fseg_gran_zeroed = nullptr;  // the granule block whose tags have been cleared (a fresh block holds anything)
  size_t fseg_gran_zeroed_bytes = 0;
  unsigned int fseg_epoch = 0;
  int fseg_poll_budget = gs::kFwdPollBudget, fseg_thin_layer = gs::kFwdThinLayerDefault;
  double fseg_gate = -1.0;  // < 0: GSPLAT_FWD_SEGMENTS_GATE / its default
  unsigned long long n_segmented_forwards = 0;
  // r06: the figures the segment kernels publish, as the host last took them from a slot whose ticket it could trust
  // (gs::take_figures)
  gs::Figures fig;
  int seg_cap = 0;          // extra segments the recorded forward had room for
  bool seg_ready = false;   // the recorded forward wrote the table and the checkpoints
  unsigned long long n_segmented_backwards = 0;
  const unsigned char *last_mask = nullptr;  // the mask array the last COMPLETED forward wrote (gsplat_context_last_compaction)
  int *h_words = nullptr;  // pinned
  bool dense_route = false;  // binning route of the next forward (follows the last one's density)
  int forced_route = 0;      // gsplat_context_set_binning_route: 0 auto, 1 counting sort, 2 radix sorts
  bool rows_ready = false;  // gsplat_backward_render has filled grad_rows for the recorded forward
  bool backward_seen = false, rows_zeroed = false;  // training use: the forward clears grad_rows for the backward
  bool render_only = false;  // gsplat_context_set_render_only: forwards skip what only a backward would read
  bool lean = false;         // gsplat_context_set_lean_forward: Sigma / J / conic / colour are not materialised
  // r06: the per-gaussian forward: 0 one fused kernel (r01-r05), 1 sh_colour_kernel then preprocess_geom_kernel on the
  // caller's stream, 2 sh_colour_kernel BESIDE preprocess_geom_kernel on a stream of the context (pre_side) -- a stream
  // of memory requests next to a kernel bound by its arithmetic (gsplat_context_set_preprocess_split)
  int pre_split = gs::pre_split_default();
  hipStream_t pre_side = nullptr;
  hipEvent_t ev_pre_fork = nullptr, ev_pre_join = nullptr;
  gs::DeviceBuffer chunk_first;  // [chunks of the index space]: slice-local rank of each chunk's first index (mode 2)
  gs::DeviceBuffer kept;     // slice-local lists of the kept gaussians (project_cull -> preprocess' compacted walk)
  gs::DeviceBuffer dir_grad;  // [M,3]: sh_adam_dir_kernel -> preprocess_bwd_kernel<L, 3> (gsplat_adam_fused.mode 2)
  gs::DeviceBuffer cam_rows;  // [ceil(M/64),16] doubles: preprocess_bwd_kernel<.., kCamGrad> -> cam_grad_finalize_kernel
  // The SH direction sums (gsplat_context_set_dir_sums; gs_math.h: sh_dir_sums): [max_gaussians,9], compacted order, written
  // by preprocess_kernel<.., kDirSums> and read by preprocess_bwd_kernel<.., kDirSums> instead of the SH rows, band 0 and
  // xyz_c.  Allocated by the first forward that writes them (never by a render-only context).  dir_sums_of names the
  // forward whose sums the buffer holds: its ticket (0: nobody's) and the inputs the sums were formed from --
  // a backward reads them only when all of that is the recorded forward's and its own; gsplat_rasterize_image voids the
  // record before it queues anything, and only the launch of the kernel that writes the sums sets it.
  gs::DeviceBuffer dir_sums;
  bool dir_sums_on = true;  // the switch; read by the next forward and by every backward (GSPLAT_NO_DIR_SUMS=1 overrides it)
  struct DirSumsOf {
    unsigned long long ticket = 0;
    const float *xyz = nullptr, *rgb = nullptr, *sh = nullptr, *view = nullptr;
    float campos[3] = {0.f, 0.f, 0.f};
  } dir_sums_of;
  unsigned long long fwd_ticket = 0;  // the recorded forward's ticket
  long long n_dir_sums_backwards = 0, n_dir_sums_fallbacks = 0;  // per-gaussian backwards that read the sums / the rows
  gs::SortFork fork;         // side streams for the per-tile sorts of long lists (created when a forward first needs them)
  // the forward's record (gs_common.h: publish_record): pinned host memory the GPU writes and the host polls
  volatile unsigned long long *h_pub = nullptr;
  unsigned long long *d_pub = nullptr, ticket = 0;
  // small device counters: 64 spread counters of candidate pairs, then the kBinBlocks slice counts of the cull
  unsigned long long *pair_counters() const { return counters.as<unsigned long long>(); }
  int *slice_counts() const { return counters.as<int>() + 128; }
  int *fseg_fallbacks() const { return counters.as<int>() + 128 + gs::kBinBlocks; }  // (zeroed at creation, then only added to)
  // optional per-stage HIP-event timing (gsplat_context_set_timing)
  static constexpr int kStages = 8, kSlots = 32;
  unsigned int timing = 0;  // bit k: stage k is timed
  hipEvent_t ev[kSlots][2 * kStages] = {};
  unsigned char pending[kSlots][kStages] = {};
  double stage_ms[kStages] = {};
  long long stage_n[kStages] = {};
  long long fwd_calls = 0;
  // what the speculative forward did (gsplat_context_get_counters): forwards, forwards whose queued tail had to be redone
  // (instances outgrew the room, or the longest list needed a sort kernel that was not queued), forwards that walked the
  // compacted slots, growths of the instance buffers
  long long n_forwards = 0, n_tail_redone = 0, n_compact_walks = 0, n_instance_growths = 0, n_ordered_backwards = 0;
  int slot = 0;
  void mark(int stage, bool stop, hipStream_t st) {
    if (!((timing >> stage) & 1u)) return;
    (void)hipEventRecord(ev[slot][2 * stage + (stop ? 1 : 0)], st);
    if (stop) pending[slot][stage] = 1;
  }
  void harvest(int sl) {
    for (int k = 0; k < kStages; ++k)
      if (pending[sl][k]) {
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, ev[sl][2 * k], ev[sl][2 * k + 1]) == hipSuccess) { stage_ms[k] += ms; stage_n[k] += 1; }
        pending[sl][k] = 0;
      }
  }
  // state of the last forward
  int N = 0, M = 0, l_max = 0, width = 0, height = 0;
  float tan_fovx = 0.f, tan_fovy = 0.f, mh_dist = 0.f;  // what the per-gaussian backward needs to redo Sigma, J, conic
  size_t S = 0;
  long long last_longest = -1;  // longest tile list of the last counting-sort forward (-1: unknown)
  bool have_forward = false;
  // the last forward completed and its records, lists, stop indices and compact_to_global are still this context's: what
  // gsplat_context_accumulate_contributions replays (true after a render-only forward too, which leaves no have_forward)
  bool lists_ready = false;
  // ---- the context's device buffers, each named ONCE: bytes(), release(), forward_outputs() and the pooled marking of
  // gsplat_context_create are loops over this table.  A new buffer is its declaration above and one line here.
  // kCounted: part of gsplat_context_bytes.  kOutput: one of the thirteen arrays of the reference's ForwardPassData
  // (cuda_data.cuh:70-86), in that order -- pooled buffers, so that gsplat_context_detach_forward_outputs can hand their
  // blocks to the caller instead of the caller copying them (r05).
  enum : unsigned { kCounted = 1u, kOutput = 2u };
  template <class C, class F>
  static void each_buffer(C &c, F &&f) {
    constexpr unsigned W = kCounted, O = kCounted | kOutput;
    f(c.mask, O); f(c.uv_all, O); f(c.xyz_c_all, O); f(c.sigma, O); f(c.conic, O); f(c.J, O); f(c.rgb, O); f(c.radius, O);
    f(c.sorted, O); f(c.ranges, O); f(c.image, O); f(c.T_px, O); f(c.n_px, O);
    f(c.counters, W); f(c.rank, W); f(c.c2g, W); f(c.xyz_c, W); f(c.uv, W); f(c.recs, W); f(c.counts, W); f(c.offsets, W);
    f(c.grad_rows, W); f(c.hitmask, W); f(c.keys_a, W); f(c.keys_b, W); f(c.pay_a, W); f(c.pay_b, W); f(c.temp, W);
    f(c.bin_table, 0u);  // released, not counted: as before this table (whether to count it is a change of its own)
    f(c.blockmasks, W); f(c.kept, W); f(c.tile_tops, W); f(c.tile_order, W);
    f(c.ids_c, W); f(c.masks_c, W); f(c.n_c_px, W); f(c.tile_useful, W);
    f(c.seg_first, W); f(c.seg_extra, W); f(c.seg_chk, W);
    f(c.fseg_first, W); f(c.fseg_blocks, W); f(c.fseg_gran, W); f(c.fseg_part, W); f(c.fseg_stop, W);
    f(c.dir_grad, W); f(c.cam_rows, W); f(c.dir_sums, W); f(c.depth_map, W); f(c.seg_chk_d, W); f(c.fseg_part_d, W);
    f(c.depth2_map, W); f(c.seg_chk_q, W); f(c.fseg_part_q, W);
    f(c.f3d_scale, W); f(c.f3d_opacity, W);
    f(c.chunk_first, 0u);  // released, not counted: as before this table
  }
  void forward_outputs(gs::DeviceBuffer *out[13]) {
    int n = 0;
    each_buffer(*this, [&](gs::DeviceBuffer &b, unsigned flags) { if (flags & kOutput) out[n++] = &b; });
  }
  size_t bytes() const {
    size_t total = 0;
    each_buffer(*this, [&](const gs::DeviceBuffer &b, unsigned flags) { if (flags & kCounted) total += b.bytes; });
    return total;
  }
  void release() {
    gs::pool_unwatch(&last_mask);
    last_mask = nullptr;
    each_buffer(*this, [](gs::DeviceBuffer &b, unsigned) { b.release(); });
    fseg_gran_zeroed = nullptr;
    fork.destroy();
    if (pre_side) { (void)hipStreamDestroy(pre_side); pre_side = nullptr; }
    if (ev_pre_fork) { (void)hipEventDestroy(ev_pre_fork); ev_pre_fork = nullptr; }
    if (ev_pre_join) { (void)hipEventDestroy(ev_pre_join); ev_pre_join = nullptr; }
    if (h_words) (void)hipHostFree(h_words);
    h_words = nullptr;
    if (h_pub) { (void)hipHostFree((void *)h_pub); h_pub = nullptr; d_pub = nullptr; }
    for (int a = 0; a < kSlots; ++a)
      for (int b = 0; b < 2 * kStages; ++b)
        if (ev[a][b]) { (void)hipEventDestroy(ev[a][b]); ev[a][b] = nullptr; }
  }
};

namespace gs {
// gs_context.hip.  Room of the instance buffers, in INSTANCES, and their growth to hold S of them
size_t instance_room(const gsplat_context *c);
int reserve_instances(gsplat_context *c, size_t S, int num_tiles, hipStream_t st);
}  // namespace gs
