// gs_fused.hip -- the device-resident per-view pass on a persistent workspace (gs_context.h), as the HOST sees it:
// gsplat_rasterize_image (the work of rasterize_image, cuda/raster.cu:12-136) and gsplat_backward_pass (the operator chain
// of TrainerImpl::backward_pass, cuda/trainer.cu:941-1012).  No kernel lives here: every launch is a launcher of gs_launch.h.
//
// Forward:   project_cull -> preprocess<L> (gs_preprocess.hip) -> bin_offsets -> bin_scatter -> tile_depth_sort_*
//            (gs_binning.hip) -> render_fwd (gs_render_fwd.hip): the sparse route; dense scenes and very large tile grids take
//            radix sorts.  ONE host read-back, the record bin_scatter publishes: everything behind the counts is queued
//            BEFORE the host waits for it, bounded by gs::instance_room(), and queued again if the record shows that it did
//            not fit (decisions: gs_forward_plan.h).
// Backward:  zero gradient rows -> compositing backward (64-byte row atomics, gs_render_bwd.hip) -> one fused per-gaussian
//            kernel for the whole SH / conic / Jacobian / Sigma / projection chain (gs_preprocess_bwd.hip).
// The reference runs ~20 thrust compactions, ~15 kernels and 5 blocking read-backs for the
// same work; results are laid out exactly like its ForwardPassData / GaussianGradients.
#include <cmath>
#include <algorithm>

#include "gs_context.h"
#include "gs_launch.h"
#include "gs_pergaussian_args.h"

extern "C" {

// ---- gsplat_rasterize_image: the forward as a sequence of steps.  What the steps share is gathered once per call in
// FwdCall; every decision they take is a function of gs_forward_plan.h.
struct FwdCall {
  const gsplat_gaussians *g; const gsplat_camera *cam; const gsplat_raster_config *cfg;  // the caller's, with bg, l_max, st
  float bg; hipStream_t st;
  int l_max, N, W, H, ntx, nty, num_tiles;
  float tan_fovx, tan_fovy;  // cuda/raster.cu:92-93
  bool compact;              // the per-gaussian kernels walk the compacted slots (gs::compact_walk)
  bool beside;               // the colour kernel beside the geometry kernel (pre_split 2)
  bool ro, mid;              // render only; Sigma, J, conic, colour stored for the caller / the stand-alone backward operators
  bool sums;                 // the per-gaussian kernel also writes the SH direction sums (gs_context.h: dir_sums)
  bool sparse, keys_ok;      // the counting-sort route (else the radix sorts); every depth key an ordinary positive float
  int *bin_table;            // sparse route: the per-workgroup tile histograms
  unsigned long long ticket;  // of the host record and the figure slots
  gs::DepthMaps dmap;         // depth mode: the compositing kernels' depth instantiations (gs_render.h: DepthMaps)
  bool join_pending;          // pre_split 2 with the late join: the colour kernel is waited for in front of render_fwd
  bool segmented_this_forward;
};
static int check_forward_args(const gsplat_context *c, const gsplat_gaussians *g, const gsplat_camera *cam,
                              const gsplat_raster_config *cfg, int l_max) {
  static const char fn[] = "gsplat_rasterize_image";
  GS_REQUIRE_IN(fn, c && g && cam && cfg, "null argument struct");
  GS_REQUIRE_IN(fn, l_max >= 0 && l_max <= 3, "l_max must be 0..3");  // cuda/raster.cu:58-60
  const int N = g->num_gaussians, W = cam->width, H = cam->height;
  GS_REQUIRE_IN(fn, N > 0, "num_gaussians must be positive");
  if (N > c->max_gaussians || W > c->max_width || H > c->max_height || W <= 0 || H <= 0) {
    gs::set_error("gsplat_rasterize_image: %d gaussians / %dx%d exceed the context capacity %d / %dx%d", N, W, H,
                  c->max_gaussians, c->max_width, c->max_height);
    return GSPLAT_ERR_CAPACITY;
  }
  GS_REQUIRE_DEV_IN(fn, g->xyz); GS_REQUIRE_DEV_IN(fn, g->rgb); GS_REQUIRE_DEV_IN(fn, g->opacity); GS_REQUIRE_DEV_IN(fn, g->scale);
  GS_REQUIRE_DEV_IN(fn, g->quaternion); GS_REQUIRE_DEV_IN(fn, cam->view); GS_REQUIRE_DEV_IN(fn, cam->proj);
  if (l_max > 0) GS_REQUIRE_DEV_IN(fn, g->sh);
  GS_REQUIRE_IN(fn, ((uintptr_t)g->quaternion & 15) == 0, "quaternion must be 16-byte aligned");
  GS_REQUIRE_IN(fn, !(c->antialiased && c->pre_split),
                "anti-aliased mode has no two-kernel forward (gsplat_context_set_preprocess_split / GSPLAT_PRE_SPLIT must be 0)");
  GS_REQUIRE_IN(fn, N <= (64 << 20), "more than 64 Mi gaussians: the cull's per-slice ballots would not fit its LDS");
  return GSPLAT_OK;
}

// The recorded forward is void from here on; outputs the caller took over (gsplat_context_detach_forward_outputs) come
// back from the pool, at their old sizes
static int reclaim_outputs(gsplat_context *c, hipStream_t st) {
  c->have_forward = c->lists_ready = c->rows_ready = c->order_ready = c->depth_ready = c->rows_depth = c->rows_abs = false;
  c->depth_inverse_ready = c->depth_moment_ready = false;
  c->dir_sums_of.ticket = 0;  // nobody's: only the launch of a kernel that writes the sums names a forward again
  gs::pool_unwatch(&c->last_mask);
  c->last_mask = nullptr;  // rank[] and compact_to_global are about to be overwritten
  gs::DeviceBuffer *outs[13];
  c->forward_outputs(outs);
  for (gs::DeviceBuffer *b : outs)
    if (b->ptr == nullptr) {
      const int r = b->reserve_again(st);  // (ordered behind the stream that returned the block, if another)
      if (r) return r;
      // a fresh `sorted` must hold valid gaussian ids wherever the speculative tail may read it (reserve_instances)
      if (b == &c->sorted) GS_HIP(hipMemsetAsync(b->ptr, 0, b->bytes, st));
    }
  return GSPLAT_OK;
}

// Everything the call decides before its first launch, and the buffers / side stream those decisions need
static int plan_forward_call(gsplat_context *c, const gsplat_gaussians *g, const gsplat_camera *cam,
                             const gsplat_raster_config *cfg, float bg_color, int l_max, hipStream_t st, FwdCall &f) {
  int rc = GSPLAT_OK;
  f = {}; f.g = g; f.cam = cam; f.cfg = cfg; f.bg = bg_color; f.l_max = l_max; f.st = st;
  f.N = g->num_gaussians; f.W = cam->width; f.H = cam->height;
  f.ntx = (f.W + 15) / 16; f.nty = (f.H + 15) / 16; f.num_tiles = f.ntx * f.nty;
  f.tan_fovx = (float)f.W / (2.0f * cam->focal_x); f.tan_fovy = (float)f.H / (2.0f * cam->focal_y);
  if (c->depth) {  // z from the compacted xyz_c, which preprocess writes in every mode
    if ((rc = c->depth_map.reserve((size_t)f.W * f.H * sizeof(float), st))) return rc;
    f.dmap.xyz_c = c->xyz_c.as<float>(); f.dmap.depth = c->depth_map.as<float>();
    f.dmap.inverse = c->depth_inverse; f.dmap.moment = c->depth_moment;
    if (c->depth_moment) {
      if ((rc = c->depth2_map.reserve((size_t)f.W * f.H * sizeof(float), st))) return rc;
      f.dmap.depth2 = c->depth2_map.as<float>();
    }
  }
  f.compact = gs::compact_walk(c->N, c->M, f.N);
  if (f.compact && (rc = c->kept.reserve((size_t)c->max_gaussians * sizeof(int)))) return rc;
  // the colour kernel beside the geometry kernel (pre_split 2): its stream and the two events, made on first use
  f.beside = c->pre_split == 2 && l_max > 0;
  if (f.beside) {
    if ((rc = c->chunk_first.reserve(((size_t)gs::bin_chunks(c->max_gaussians) + gs::kBinThreads / 64 + 1) * sizeof(int)))) return rc;
    if (!c->pre_side) {
      int lo_prio = 0, hi_prio = 0;
      GS_HIP(hipDeviceGetStreamPriorityRange(&lo_prio, &hi_prio));  // (numerically largest = lowest priority)
      GS_HIP(hipStreamCreateWithPriority(&c->pre_side, hipStreamNonBlocking, lo_prio));
      GS_HIP(hipEventCreateWithFlags(&c->ev_pre_fork, hipEventDisableTiming));
      GS_HIP(hipEventCreateWithFlags(&c->ev_pre_join, hipEventDisableTiming));
    }
  }
  f.ro = c->render_only; f.mid = !f.ro && !c->lean;
  // the direction sums: written by the one fused kernel only -- the two-kernel forms and the anti-aliased form have no
  // such instantiation, and a forward nobody differentiates needs none.  Not at degree 0 either: there is no row to save,
  // the sums (36 B) are more than the band 0 and xyz_c (24 B) they would replace, and a forward-only caller would pay for
  // the stores (config2: +0.8 us of 78 with them)
  f.sums = c->dir_sums_on && !gs::no_dir_sums() && l_max > 0 && !f.ro && c->pre_split == 0 && !c->antialiased;
  if (f.sums && (rc = c->dir_sums.reserve((size_t)c->max_gaussians * 9 * sizeof(float), st))) return rc;
  // Two binning routes, both exact for any scene; the choice only affects speed, so it follows the LAST forward's
  // density (the first call starts sparse): sparse = LDS counting sort + per-tile depth sort, dense (more than
  // ~768 list entries per tile) or very large tile grids = stable radix sorts (gs_binning.hip).
  const bool want_dense = c->forced_route == 2 || (c->forced_route == 0 && c->dense_route);
  f.sparse = !want_dense && gs::binning_supports_counting_sort(f.num_tiles);
  if (f.sparse) {
    if ((rc = c->bin_table.reserve(gs::binning_table_bytes(f.num_tiles)))) return rc;
    f.bin_table = c->bin_table.as<int>();
  }
  f.keys_ok = cfg->near_thresh >= 1e-30f; f.ticket = ++c->ticket;
  return GSPLAT_OK;
}

static int launch_cull(gsplat_context *c, const FwdCall &f) {
  c->mark(0, false, f.st);
  gs::CullArgs a = {};
  a.xyz = f.g->xyz; a.view = f.cam->view; a.proj = f.cam->proj;
  a.N = f.N; a.width = f.W; a.height = f.H;
  a.near_thresh = f.cfg->near_thresh; a.padding = f.cfg->cull_mask_padding;
  if (!c->lean) { a.xyz_c = c->xyz_c_all.as<float>(); a.uv = c->uv_all.as<float>(); }
  a.mask = c->mask.as<unsigned char>(); a.rank = c->rank.as<int>();
  a.slice_counts = c->slice_counts(); a.pair_counters = c->pair_counters();
  if (f.compact) a.kept = c->kept.as<int>();
  if (f.beside && !f.compact) a.chunk_first = c->chunk_first.as<int>();
  if (int rc = gs::launch_project_cull(a, f.st)) return rc;
  c->mark(0, true, f.st);
  return GSPLAT_OK;
}

// the colour kernel of the two-kernel forms (see sh_colour_kernel), on stream `cst`
static int launch_colour(gsplat_context *c, const FwdCall &f, hipStream_t cst) {
  if (f.l_max == 0) return GSPLAT_OK;
  gs::ShColourArgs a = {};
  a.g = *f.g;
  a.mask = c->mask.as<unsigned char>();
  a.slice_counts = c->slice_counts();
  if (f.compact) a.kept = c->kept.as<int>();
  else a.chunk_first = c->chunk_first.as<int>();
  for (int k = 0; k < 3; ++k) a.campos[k] = f.cam->campos[k];
  if (f.beside) {  // rank[] is being rewritten next door; the colour goes straight into the records
    if (f.mid) a.rgb_out = c->rgb.as<float>();
    a.recs = c->recs.as<float4>();
  } else {
    a.rank = c->rank.as<int>();
    a.rgb_out = c->rgb.as<float>();
  }
  a.l_max = f.l_max; a.compact = f.compact;
  return gs::launch_sh_colour(a, cst);
}

// Everything per kept gaussian: the fused kernel, or the two split forms (r06: colour and geometry as two kernels, one
// behind the other or side by side; see sh_colour_kernel)
static int launch_per_gaussian(gsplat_context *c, FwdCall &f) {
  hipStream_t st = f.st;
  int rc = GSPLAT_OK;
  c->mark(1, false, st);
  const bool mid = f.mid;
  gs::PreprocessArgs a = {};
  a.g = *f.g; a.view = f.cam->view; a.proj = f.cam->proj;
  a.mask = c->mask.as<unsigned char>(); a.rank = c->rank.as<int>();
  a.slice_counts = c->slice_counts(); a.kept = c->kept.as<int>();
  a.width = f.W; a.height = f.H; a.ntx = f.ntx; a.nty = f.nty;
  a.fx = f.cam->focal_x; a.fy = f.cam->focal_y; a.tan_fovx = f.tan_fovx; a.tan_fovy = f.tan_fovy;
  a.mh_dist = f.cfg->mh_dist;
  for (int k = 0; k < 3; ++k) a.campos[k] = f.cam->campos[k];
  a.c2g = c->c2g.as<int>(); a.xyz_c = c->xyz_c.as<float>(); a.uv = c->uv.as<float>();
  if (mid) { a.sigma = c->sigma.as<float>(); a.conic = c->conic.as<float>(); a.J = c->J.as<float>(); a.rgb = c->rgb.as<float>(); }
  a.radius = c->radius.as<float>(); a.recs = c->recs.as<float4>(); a.counts = c->counts.as<int>();
  a.hitmask = c->hitmask.as<unsigned long long>(); a.pairs = c->pair_counters();
  a.table = f.bin_table;
  a.l_max = f.l_max; a.store_mid = mid; a.compact = f.compact; a.antialiased = c->antialiased;
  if (c->pre_split) {
    const bool seq = f.l_max > 0 && c->pre_split == 1;  // one behind the other: the colour travels through c->rgb
    if (seq) a.rgb = c->rgb.as<float>();
    hipStream_t cst = st;
    if (f.beside) {  // the colour kernel's stream starts where the cull has finished
      GS_HIP(hipEventRecord(c->ev_pre_fork, st));
      GS_HIP(hipStreamWaitEvent(c->pre_side, c->ev_pre_fork, 0));
      cst = c->pre_side;
    }
    if (seq && (rc = launch_colour(c, f, cst))) return rc;
    // (the geometry kernel is queued FIRST: its 256 workgroups want a CU each, the colour kernel's take what is left)
    if ((rc = gs::launch_preprocess_geom(a, f.l_max == 0 ? 0 : f.beside ? 2 : 1, st))) return rc;
    if (f.beside) {
      if ((rc = launch_colour(c, f, cst))) return rc;
      GS_HIP(hipEventRecord(c->ev_pre_join, c->pre_side));
      if (gs::pre_join_late()) f.join_pending = true;
      else GS_HIP(hipStreamWaitEvent(st, c->ev_pre_join, 0));
    }
  } else {
    if (f.sums) a.dir_sums = c->dir_sums.as<float>();
    if ((rc = gs::launch_preprocess(a, st))) return rc;
    if (f.sums) {  // the buffer now holds this forward's sums, of these inputs
      gsplat_context::DirSumsOf &of = c->dir_sums_of;
      of.ticket = f.ticket;
      of.xyz = f.g->xyz; of.rgb = f.g->rgb; of.sh = f.g->sh; of.view = f.cam->view;
      for (int k = 0; k < 3; ++k) of.campos[k] = f.cam->campos[k];
    }
  }
  c->fwd_antialiased = c->antialiased;
  return GSPLAT_OK;
}

// Counts -> offsets for either route, and on the radix route the record and the emit.  Nothing here needs the totals on
// the host, only room for its writes: `room` is what the kernels queued before the wait may use of ALL the instance
// buffers (instance_room), and the host sleeps on the read-back while they run (the reference blocks five times, GPU idle).
static int queue_counts(gsplat_context *c, const FwdCall &f, size_t &room) {
  const int N = f.N; hipStream_t st = f.st;
  int rc = GSPLAT_OK;
  if (f.sparse) {
    if (gs::instance_room(c) < 2 && (rc = gs::reserve_instances(c, 4 * (size_t)N, f.num_tiles, st))) return rc;
    room = gs::instance_room(c) - 1;
    c->mark(1, true, st);
    c->mark(2, false, st);
    return gs::binning_offsets(f.ntx, f.nty, f.bin_table, c->keys_a.as<int>(), st);
  }
  rc = gs::scan_counts(N, c->counts.as<int>(), c->offsets.as<int>(), c->temp.ptr, c->temp.bytes, st);
  if (rc) return rc;
  c->mark(1, true, st);
  if ((rc = gs::launch_publish_counts(c->rank.as<int>() + N, c->offsets.as<int>() + N, c->pair_counters(), c->d_pub, f.ticket, st)))
    return rc;
  if (gs::instance_room(c) < 2 && (rc = gs::reserve_instances(c, 4 * (size_t)N, f.num_tiles, st))) return rc;
  room = gs::instance_room(c) - 1;
  c->mark(2, false, st);
  return gs::launch_tile_emit(c->uv.as<float>(), c->xyz_c.as<float>(), c->radius.as<float>(), f.ntx, f.nty, N,
                              c->mask.as<unsigned char>(), c->rank.as<int>(), c->offsets.as<int>(),
                              c->hitmask.as<unsigned long long>(), (long long)room, c->keys_a.as<unsigned int>(),
                              c->pay_a.as<unsigned long long>(), st);
}

// The context's arrays as the compositing kernels' option structs (gs_render.h).  The backward's split lists with room
// for `extra_cap` further segments: the forward that writes the checkpoints adds what it publishes (asked, stats, tag)
static gs::TileSegments backward_segments(gsplat_context *c, int extra_cap) {
  gs::TileSegments seg = {};
  seg.granted = c->seg_first.as<int>();
  seg.extra = c->seg_extra.as<int2>();
  seg.extra_count = reinterpret_cast<int *>(seg.extra + extra_cap);  // [extra_cap]: the count
  seg.chk = c->seg_chk.as<float4>();
  seg.image = c->image.as<float>();
  seg.extra_cap = extra_cap;
  return seg;
}
// What both routes' render_fwd launches share: the records and lists in, the per-pixel arrays out, the gradient rows to
// clear on the side (`zero_vec` float4), the block masks unless the forward only renders, and depth mode
static gs::RenderFwdArgs packed_forward_args(gsplat_context *c, const FwdCall &f, long long zero_vec) {
  gs::RenderFwdArgs a = {};
  a.recs = c->recs.as<float4>();
  a.sorted = c->sorted.as<int>();
  a.ranges = c->ranges.as<int>();
  a.width = f.W; a.height = f.H; a.bg = f.bg;
  a.n_out = c->n_px.as<int>();
  a.T_out = c->T_px.as<float>();
  a.image = c->image.as<float>();
  if (c->rows_zeroed) a.zero = c->grad_rows.as<float4>();
  a.zero_vec = zero_vec;
  if (!f.ro) a.masks_out = c->blockmasks.as<unsigned short>();
  a.depth = f.dmap;  // ({} unless the context renders depth)
  return a;
}
static gs::CompactLists compact_lists(gsplat_context *c) {
  gs::CompactLists cl = {};
  cl.ids = c->ids_c.as<int>();
  cl.masks = c->masks_c.as<unsigned short>();
  cl.n_px = c->n_c_px.as<int>();
  cl.count = c->tile_useful.as<int>();
  return cl;
}

// Sparse route: placement, per-tile sorts and render_fwd, queued before the host knows S (gs::tail_needs_redo has the
// protocol) and bounded by `cap`: `ranges` on the device are clamped to it (bin_scatter_kernel), so whatever S turns out
// to be, the kernels stay inside the buffers.  Which long-list kernels to queue follows `longest_hint`; a forward whose
// tail has to be redone comes through here again, with the true S and longest list.  `publish`: the placement
// publishes the record.
static int queue_sparse_tail(gsplat_context *c, FwdCall &f, size_t cap, long long longest_hint, bool publish) {
  const int num_tiles = f.num_tiles; const bool ro = f.ro; hipStream_t st = f.st;
  if (cap + 1 > gs::instance_room(c)) {  // every kernel below indexes the instance arrays up to `cap` (inclusive: the spare slot)
    gs::set_error("gsplat_rasterize_image: internal: %zu instances queued into room for %zu", cap, gs::instance_room(c));
    return GSPLAT_ERR_CAPACITY;
  }
  if ((longest_hint < 0 || longest_hint > 2048) && !c->fork.ready) {  // lists beyond two register-sorted runs: see SortFork
    const int fr = c->fork.create();
    if (fr) return fr;
  }
  int r = gs::binning_scatter_and_sort(c->uv.as<float>(), c->xyz_c.as<float>(), c->radius.as<float>(),
                                       c->hitmask.as<unsigned long long>(), c->rank.as<int>(), f.N, f.ntx, f.nty,
                                       c->bin_table.as<int>(), c->ranges.as<int>(), cap, c->pay_a.as<unsigned long long>(),
                                       c->keys_a.as<int>(), c->sorted.as<int>(), longest_hint, c->rank.as<int>() + f.N,
                                       c->pair_counters(), publish ? c->d_pub : nullptr, f.ticket, st, &c->fork, f.compact,
                                       f.keys_ok);
  if (r) return r;
  c->mark(2, true, st);
  c->mark(4, false, st);
  // Everything below is decided, like the kernels queued above, by the previous forward's figures (the rules and what
  // they were measured against: gs_forward_plan.h).  Heaviest-first tiles for the backward:
  const bool ordered = !ro && gs::tile_order_supported(num_tiles) && !gs::no_tile_order() &&
                       gs::tile_order_pays(c->last_longest, num_tiles, c->S);
  // Lists beyond kSegSplitMin are split for the backward (gs_render.h: TileSegments): the previous forward's longest list
  // says whether there is anything to split; the room for extra blocks follows what its tiles asked for (a list that
  // does not fit stays whole).  The figures the segment kernels publish (gs::take_figures):
  const volatile unsigned long long *h_slot = c->h_pub + 8 + 4 * (f.ticket & 1ull);
  unsigned long long w[4];
  for (int k = 0; k < 4; ++k) w[k] = __atomic_load_n(&h_slot[k], __ATOMIC_RELAXED);
  gs::take_figures(w, f.ticket, c->fig);
  unsigned long long *d_slot = c->d_pub + 8 + 4 * (f.ticket & 1ull);  // where THIS forward's kernels publish
  const unsigned int my_tag = (unsigned int)(f.ticket & 0xFFFFFFFFull);
  gs::TileSegments seg = {};
  seg.tag = my_tag;
  const bool split = !ro && !gs::no_segments() && c->last_longest > gs::kSegSplitMin && num_tiles <= 16384;  // (the table kernels' reach)
  if (split) {
    const size_t slots = cap / gs::kSegEntries + 2;  // (gs_render.h: segment_slot)
    const size_t want = gs::bwd_segment_room(cap, (size_t)c->fig.asked_bwd, gs::kSegEntries);
    if ((r = c->seg_first.reserve(((size_t)num_tiles + 8) * 4))) return r;
    if ((r = c->seg_extra.reserve((want + 2) * sizeof(int2)))) return r;  // [want]: the count
    if ((r = c->seg_chk.reserve(slots * 256 * sizeof(float4)))) return r;
    if (c->depth && (r = c->seg_chk_d.reserve(slots * 256 * sizeof(float)))) return r;
    if (c->depth && c->depth_moment && (r = c->seg_chk_q.reserve(slots * 256 * sizeof(float)))) return r;
    seg = backward_segments(c, (int)want);
    seg.asked = d_slot + 2;
    seg.tag = my_tag;
  }
  // the tiles' largest stop indices of this forward, for the next one's decision below
  const bool figures = !gs::no_fwd_segments() && c->last_longest > gs::kSegSplitMin && num_tiles <= 16384;
  if (figures) seg.stats = d_slot;
  // ... and for the forward itself (gs_render.h: FwdSegments): every segment of a long list a block of its own, only
  // where the tiles' work is uneven enough
  gs::FwdSegments fs = {};
  const double gate = c->fseg_gate >= 0.0 ? c->fseg_gate : gs::fwd_segments_gate();
  const bool fsplit = figures && gs::forward_split_pays(c->fig.max, c->fig.sum, gate);
  if (fsplit) {
    const size_t want = gs::fwd_segment_room(cap, num_tiles, (size_t)c->fig.asked_fwd, gs::kSegEntries);
    if ((r = c->fseg_first.reserve(((size_t)num_tiles + 8 + 136) * 4))) return r;  // ranks | layer bases
    if ((r = c->fseg_blocks.reserve((want + 2) * sizeof(int2)))) return r;  // [want]: the count
    if ((r = c->fseg_gran.reserve(2 * want * 256 * sizeof(unsigned long long)))) return r;  // t products | final Ts
    if ((r = c->fseg_part.reserve(want * 256 * sizeof(float4)))) return r;
    if (c->depth && (r = c->fseg_part_d.reserve(want * 256 * sizeof(float)))) return r;
    if (c->depth && c->depth_moment && (r = c->fseg_part_q.reserve(want * 256 * sizeof(float)))) return r;
    if ((r = c->fseg_stop.reserve(want * 256 * sizeof(int)))) return r;
    if (c->fseg_gran.ptr != c->fseg_gran_zeroed || c->fseg_gran.bytes != c->fseg_gran_zeroed_bytes) {
      GS_HIP(hipMemsetAsync(c->fseg_gran.ptr, 0, c->fseg_gran.bytes, st));  // tags of no epoch
      c->fseg_gran_zeroed = c->fseg_gran.ptr;
      c->fseg_gran_zeroed_bytes = c->fseg_gran.bytes;
    }
    if (++c->fseg_epoch == 0) c->fseg_epoch = 1;
    fs.rank = c->fseg_first.as<int>();
    fs.base = fs.rank + num_tiles + 8;
    fs.blocks = c->fseg_blocks.as<int2>();
    fs.count = reinterpret_cast<int *>(fs.blocks + want);
    fs.granules = c->fseg_gran.as<unsigned long long>();
    fs.part = c->fseg_part.as<float4>();
    fs.stop = c->fseg_stop.as<int>();
    fs.cap = (int)want;
    fs.epoch = c->fseg_epoch;
    fs.asked = d_slot + 3;
    fs.tag = my_tag;
    fs.fallbacks = c->fseg_fallbacks();
    fs.poll_budget = c->fseg_poll_budget;
    fs.thin_layer = c->fseg_thin_layer;
    if ((r = gs::launch_fwd_segments_table(c->ranges.as<int>(), num_tiles, fs, st))) return r;
    f.segmented_this_forward = true;  // (counted once per forward: a redone tail comes through here twice)
  }
  if (f.join_pending) GS_HIP(hipStreamWaitEvent(st, c->ev_pre_join, 0));  // (late join: the records' colour is first read here)
  gs::RenderFwdArgs a = packed_forward_args(c, f, (long long)f.N * 4);  // M <= N is not known here yet
  if (c->depth) {
    a.depth.chk = split ? c->seg_chk_d.as<float>() : nullptr;
    a.depth.part = fsplit ? c->fseg_part_d.as<float>() : nullptr;
    if (c->depth_moment) {
      a.depth.chk2 = split ? c->seg_chk_q.as<float>() : nullptr;
      a.depth.part2 = fsplit ? c->fseg_part_q.as<float>() : nullptr;
    }
  }
  // Compact lists for the backward (gs_render.h: CompactLists): the one-workgroup-per-tile forward of a training context
  // writes them; a context that has seen a list beyond kSegSplitMin keeps the segment paths as they are.
  const bool compact = !ro && c->compact_lists && !gs::no_compact_lists() && !split && !figures && !fsplit;
  if (ordered || split || figures) a.tops_out = c->tile_tops.as<int>();
  if (split) a.segments = seg;  // (without a split the kernel sees none of seg: its tag and stats are launch_tile_segments')
  a.fwd_segments = fs;
  if (compact) a.compact = compact_lists(c);
  if ((r = gs::launch_render_fwd(a, st))) return r;
  c->compact_written = compact;
  c->seg_ready = split;
  c->seg_cap = seg.extra_cap;
  c->mark(4, true, st);
  // the backward's tile order, behind the forward: nothing waits for it until the loss has produced dL/dimage
  if (ordered && (r = gs::launch_tile_order(c->tile_tops.as<int>(), nullptr, num_tiles, c->tile_order.as<int>(), st))) return r;
  c->order_ready = ordered;
  // ... and which segments of the long lists get a block of their own
  if ((split || figures) && (r = gs::launch_tile_segments(c->ranges.as<int>(), c->tile_tops.as<int>(), num_tiles, seg, st))) return r;
  return GSPLAT_OK;
}

// The one host read-back of the forward: poll the mapped record; every few hundred polls ask the runtime about the
// stream, which both keeps its submission path moving and tells us when everything queued so far has drained.
static int wait_for_record(gsplat_context *c, const FwdCall &f, gs::ForwardRecord &rec) {
  unsigned long long w[gs::kRecordWords];
  bool drained = false;
  for (long long polls = 1;; ++polls) {
    for (int k = 0; k < gs::kRecordWords; ++k) w[k] = __atomic_load_n(&c->h_pub[k], __ATOMIC_RELAXED);
    if (gs::record_arrived(w, f.ticket)) break;
    if (drained) {  // the stream had drained before these loads: the record would be there
      gs::set_error("gsplat_rasterize_image: the count record never arrived");
      return GSPLAT_ERR_HIP;
    }
    if ((polls & 255) == 0) {
      const hipError_t q = hipStreamQuery(f.st);
      if (q != hipSuccess && q != hipErrorNotReady) {
        gs::set_error("gsplat_rasterize_image: %s while waiting for the counts", hipGetErrorString(q));
        return GSPLAT_ERR_HIP;
      }
      if ((drained = q == hipSuccess)) continue;  // look once more, at once
    }
    __builtin_ia32_pause();
  }
  __atomic_thread_fence(__ATOMIC_ACQUIRE);
  rec = gs::decode_record(w);
  if (!f.sparse) rec.longest = -1;  // (the radix route does not know it)
  if (rec.M == 0) {
    gs::set_error("gsplat_rasterize_image: no gaussians in view");  // cuda/raster.cu:38-41
    return GSPLAT_ERR_NO_VISIBLE;
  }
  return GSPLAT_OK;
}

// Radix route behind the record: grow the instance buffers if S outgrew them (synchronises) and emit again; sort, ranges, compositing
static int finish_radix_route(gsplat_context *c, const FwdCall &f, const gs::ForwardRecord &rec, size_t inst_cap) {
  const size_t S = rec.S; hipStream_t st = f.st;
  int rc = gs::reserve_instances(c, S, f.num_tiles, st);
  if (rc) return rc;
  if (S + 1 > gs::instance_room(c)) {
    gs::set_error("gsplat_rasterize_image: internal: %zu instances sorted in room for %zu", S, gs::instance_room(c));
    return GSPLAT_ERR_CAPACITY;
  }
  rc = gs::emit_sort_ranges(c->uv.as<float>(), c->xyz_c.as<float>(), c->radius.as<float>(), f.ntx, f.nty, f.N,
                            c->mask.as<unsigned char>(), c->rank.as<int>(), c->offsets.as<int>(), S,
                            c->keys_a.as<unsigned int>(), c->keys_b.as<unsigned int>(),
                            c->pay_a.as<unsigned long long>(), c->pay_b.as<unsigned long long>(),
                            c->sorted.as<int>(), c->ranges.as<int>(), c->temp.ptr, c->temp.bytes, st, S <= inst_cap,
                            c->hitmask.as<unsigned long long>());
  if (rc) return rc;
  c->mark(2, true, st);
  c->mark(4, false, st);
  if (f.join_pending) GS_HIP(hipStreamWaitEvent(st, c->ev_pre_join, 0));
  // (no tile order on this route: the longest list is not known; see queue_sparse_tail)
  if ((rc = gs::launch_render_fwd(packed_forward_args(c, f, (long long)rec.M * 4), st))) return rc;
  c->compact_written = false;  // (the longest list is not known on this route: its backwards walk the full lists)
  c->seg_ready = false;
  c->mark(4, true, st);
  c->order_ready = false;
  return GSPLAT_OK;
}

// The forward is recorded in the context (what the backward entry points check against) and described to the caller
static void record_forward(gsplat_context *c, const FwdCall &f, const gs::ForwardRecord &rec, gsplat_forward_view *out) {
  if (f.segmented_this_forward) c->n_segmented_forwards++;
  c->N = f.N; c->M = rec.M; c->S = rec.S; c->l_max = f.l_max; c->width = f.W; c->height = f.H;
  c->last_mask = c->mask.as<unsigned char>();
  gs::pool_watch(c->last_mask, &c->last_mask);  // cleared when whoever ends up owning the block returns it to the pool
  c->tan_fovx = f.tan_fovx; c->tan_fovy = f.tan_fovy; c->mh_dist = f.cfg->mh_dist;
  c->have_forward = !f.ro;  // a render-only forward leaves nothing for a backward
  c->fwd_ticket = f.ticket;
  c->lists_ready = true;
  c->depth_ready = c->depth;
  c->depth_inverse_ready = c->depth && f.dmap.inverse;
  c->depth_moment_ready = c->depth && f.dmap.moment;
  if (!out) return;
  const bool mid = f.mid;
  out->num_culled = (size_t)rec.M; out->num_pairs = (size_t)rec.pairs; out->num_splats = rec.S;
  out->mask = c->mask.as<unsigned char>(); out->compact_to_global = c->c2g.as<int>();
  out->uv = c->lean ? nullptr : c->uv_all.as<float>(); out->xyz_c = c->lean ? nullptr : c->xyz_c_all.as<float>();
  out->sigma = mid ? c->sigma.as<float>() : nullptr; out->conic = mid ? c->conic.as<float>() : nullptr;
  out->J = mid ? c->J.as<float>() : nullptr; out->precomputed_rgb = mid ? c->rgb.as<float>() : nullptr;
  out->radius = c->radius.as<float>(); out->uv_selected = c->uv.as<float>(); out->xyz_c_selected = c->xyz_c.as<float>();
  out->sorted_gaussians = c->sorted.as<int>(); out->splat_start_end_idx_by_tile_idx = c->ranges.as<int>();
  out->image = c->image.as<float>(); out->weight_per_pixel = c->T_px.as<float>();
  out->splats_per_pixel = c->n_px.as<int>();
}

int gsplat_rasterize_image(gsplat_context *c, const gsplat_gaussians *g, const gsplat_camera *cam,
                           const gsplat_raster_config *cfg, float bg_color, int l_max, gsplat_forward_view *out,
                           void *stream) {
  int rc = check_forward_args(c, g, cam, cfg, l_max);
  if (rc) return rc;
  hipStream_t st = (hipStream_t)stream;
  if ((rc = reclaim_outputs(c, st))) return rc;
  // 3D smoothing filter: the chain below runs, unchanged, on the filtered scale and opacity
  gsplat_gaussians filtered;
  if (c->filter3d) {
    GS_REQUIRE_DEV(c->filter3d);
    if ((rc = c->f3d_scale.reserve((size_t)c->max_gaussians * 3 * sizeof(float), st))) return rc;
    if ((rc = c->f3d_opacity.reserve((size_t)c->max_gaussians * sizeof(float), st))) return rc;
    if ((rc = gs::launch_filter3d_apply(g->scale, g->opacity, c->filter3d, g->num_gaussians, c->f3d_scale.as<float>(),
                                        c->f3d_opacity.as<float>(), st))) return rc;
    filtered = *g; filtered.scale = c->f3d_scale.as<float>(); filtered.opacity = c->f3d_opacity.as<float>();
    g = &filtered;
  }
  c->fwd_filter3d = c->filter3d;
  FwdCall f;
  if ((rc = plan_forward_call(c, g, cam, cfg, bg_color, l_max, st, f))) return rc;
  if (c->timing) {  // next timing slot; its events are >= kSlots forwards old, hence complete
    c->slot = (int)(c->fwd_calls % gsplat_context::kSlots);
    c->harvest(c->slot);
  }
  c->fwd_calls++;
  if ((rc = launch_cull(c, f))) return rc;
  if ((rc = launch_per_gaussian(c, f))) return rc;
  size_t room = 0;  // of the instance buffers: what the kernels queued before the wait may use
  if ((rc = queue_counts(c, f, room))) return rc;
  // once a backward has been seen, the forward clears the gradient rows on the side (see render_fwd_kernel)
  if (c->rows_zeroed) c->backward_seen = false;  // the last forward's cleared rows were never used: rendering only
  c->rows_zeroed = c->backward_seen && !f.ro;
  const long long spec_hint = f.sparse ? gs::speculative_longest(c->last_longest) : -1;
  if (f.sparse && (rc = queue_sparse_tail(c, f, room, spec_hint, true))) return rc;
  gs::ForwardRecord rec;
  if ((rc = wait_for_record(c, f, rec))) return rc;
  c->dense_route = gs::binning_next_route_is_radix(f.sparse, rec.S, f.num_tiles, rec.longest);
  c->last_longest = rec.longest;
  c->n_forwards++;
  if (f.compact) c->n_compact_walks++;
  if (!f.sparse) {
    if ((rc = finish_radix_route(c, f, rec, room))) return rc;
  } else if (gs::tail_needs_redo(rec.S, room, spec_hint, rec.longest, f.keys_ok)) {
    c->n_tail_redone++;
    c->dir_sums_of.ticket = 0;  // (a forward queued twice: its backwards take the path that reads the rows)
    if (rec.S > room) {  // grow (synchronises); the placement queued below writes the true ranges
      c->n_instance_growths++;
      if ((rc = gs::reserve_instances(c, rec.S + rec.S / 4, f.num_tiles, st))) return rc;
    }
    // the long-tile counter lives at the head of keys_a: zeroed by bin_offsets, then used by the queued sorts
    GS_HIP(hipMemsetAsync(c->keys_a.ptr, 0, sizeof(int), st));
    if ((rc = queue_sparse_tail(c, f, rec.S, rec.longest, false))) return rc;
  }
  // The backward walks the compact lists of a forward whose own longest list stayed whole: a first forward with longer
  // lists (the split follows the forward before) hands over the full lists, as it always has.
  c->compact_ready = c->compact_written && rec.longest >= 0 && rec.longest <= gs::kSegSplitMin;
  record_forward(c, f, rec, out);
  return GSPLAT_OK;
}

int gsplat_backward_render(gsplat_context *c, const float *grad_image, float bg_color, float *rgb_global,
                           void *stream) {
  return gsplat_backward_render_split(c, grad_image, bg_color, rgb_global, nullptr, nullptr, stream);
}

int gsplat_backward_render_split(gsplat_context *c, const float *grad_image, float bg_color, float *rgb_global,
                                 float *common, float *uv_norm, void *stream) {
  return gsplat_backward_render_depth2(c, grad_image, nullptr, nullptr, nullptr, bg_color, rgb_global, common, uv_norm, stream);
}

int gsplat_backward_render_depth(gsplat_context *c, const float *grad_image, const float *grad_depth,
                                 const float *grad_alpha, float bg_color, float *rgb_global, float *common, float *uv_norm,
                                 void *stream) {
  return gsplat_backward_render_depth2(c, grad_image, grad_depth, grad_alpha, nullptr, bg_color, rgb_global, common, uv_norm, stream);
}

int gsplat_backward_render_depth2(gsplat_context *c, const float *grad_image, const float *grad_depth,
                                  const float *grad_alpha, const float *grad_depth2, float bg_color, float *rgb_global,
                                  float *common, float *uv_norm, void *stream) {
  // (every check before the first launch: a refused call leaves the context and the caller's arrays as they were)
  GS_REQUIRE(c != nullptr, "null context");
  GS_REQUIRE(c->have_forward, "no forward pass recorded in this context");
  GS_REQUIRE_DEV(grad_image);
  if (rgb_global) GS_REQUIRE_DEV(rgb_global);
  if (common) {
    GS_REQUIRE(rgb_global != nullptr, "the common rows are cleared by the pass that scatters g_rgb: rgb_global is needed");
    GS_REQUIRE_DEV(common);
    GS_REQUIRE(((uintptr_t)common & 15) == 0, "common must be 16-byte aligned");
  }
  if (uv_norm) { GS_REQUIRE(common != nullptr, "uv_norm goes with common"); GS_REQUIRE_DEV(uv_norm); }
  const bool depth = grad_depth != nullptr || grad_alpha != nullptr || grad_depth2 != nullptr;  // all NULL: the plain backward, exactly
  if (grad_depth) GS_REQUIRE_DEV(grad_depth);
  if (grad_alpha) GS_REQUIRE_DEV(grad_alpha);
  if (grad_depth2) GS_REQUIRE_DEV(grad_depth2);
  GS_REQUIRE(!depth || c->depth_ready, "depth / alpha gradients need a forward that rendered depth (gsplat_context_set_depth)");
  GS_REQUIRE(!grad_depth2 || c->depth_moment_ready,
             "grad_depth2 needs a forward that rendered the second moment (gsplat_context_set_depth_mode)");
  // (a forward with the moment option runs the moment backward whichever maps are given: a null dL/dQ reads as zero)
  GS_REQUIRE(!(depth && c->depth_moment_ready && c->absgrad),
             "the moment option has no absgrad form: depth gradients of such a forward cannot be taken in absgrad mode");
  hipStream_t st = (hipStream_t)stream;
  const int M = c->M, W = c->width, H = c->height;
  c->rows_ready = false;
  c->rows_depth = false;
  c->rows_abs = false;
  c->backward_seen = true;
  if (!c->rows_zeroed) {  // first backward of the context, or a second backward of the same forward
    c->mark(5, false, st);
    GS_HIP(hipMemsetAsync(c->grad_rows.ptr, 0, (size_t)M * 64, st));
    c->mark(5, true, st);
  }
  c->rows_zeroed = false;
  // stage 6 is this one launch: when it is timed, the launch itself stamps the two events (see launch_render_bwd)
  const bool timed = (c->timing >> 6) & 1u;
  gs::RenderBwdArgs a = {};
  a.recs = c->recs.as<float4>();
  // compact lists (gs_render.h: CompactLists): the same kernel on the useful entries only -- ids, masks and stop indices
  const bool compact = c->compact_ready && !c->seg_ready;
  const gs::CompactLists cl = compact_lists(c);
  a.sorted = compact ? cl.ids : c->sorted.as<int>();
  a.masks_in = compact ? cl.masks : c->blockmasks.as<unsigned short>();
  a.n_px = compact ? cl.n_px : c->n_px.as<int>();
  a.ranges = c->ranges.as<int>();
  a.T_px = c->T_px.as<float>();
  a.grad_image = grad_image;
  a.width = W; a.height = H; a.bg = bg_color;
  a.out.rows = c->grad_rows.as<float>();
  if (c->order_ready && !gs::no_tile_order()) a.order = c->tile_order.as<int>();
  if (timed) { a.ev_start = c->ev[c->slot][12]; a.ev_stop = c->ev[c->slot][13]; }
  if (c->seg_ready) a.segments = backward_segments(c, c->seg_cap);
  if (depth) {
    a.depth.xyz_c = c->xyz_c.as<float>();
    a.depth.depth = c->depth_map.as<float>();
    if (c->seg_ready) a.depth.chk = c->seg_chk_d.as<float>();
    a.depth.grad_depth = grad_depth;
    a.depth.grad_alpha = grad_alpha;
    a.depth.inverse = c->depth_inverse_ready;
    if (c->depth_moment_ready) {
      a.depth.moment = true;
      a.depth.depth2 = c->depth2_map.as<float>();
      if (c->seg_ready) a.depth.chk2 = c->seg_chk_q.as<float>();
      a.depth.grad_depth2 = grad_depth2;
    }
  }
  a.absgrad = c->absgrad;
  const int rc = gs::launch_render_bwd(a, st);
  if (rc) return rc;
  if (c->seg_ready) c->n_segmented_backwards++;
  if (compact) c->n_compact_backwards++;
  if (c->order_ready && !gs::no_tile_order()) c->n_ordered_backwards++;
  if (timed) c->pending[c->slot][6] = 1;
  if (rgb_global) {
    const int r = gs::launch_scatter_rgb_rows(c->mask.as<unsigned char>(), c->rank.as<int>(), c->N, c->grad_rows.as<float>(),
                                              rgb_global, common, uv_norm, st);
    if (r) return r;
  }
  c->rows_ready = true;
  c->rows_depth = depth;
  c->rows_abs = c->absgrad;
  return GSPLAT_OK;
}

// ---- Checks the backward entry points share.  `fn` is the public function the caller called: the error text's prefix.
// A forward is recorded and the arguments are the ones it ran with
static int check_recorded_forward(const char *fn, const gsplat_context *c, const gsplat_gaussians *g,
                                  const gsplat_camera *cam, int l_max) {
  GS_REQUIRE_IN(fn, c->have_forward, "no forward pass recorded in this context");
  GS_REQUIRE_IN(fn, l_max == c->l_max && g->num_gaussians == c->N && cam->width == c->width && cam->height == c->height,
                "backward arguments do not match the recorded forward pass");
  return GSPLAT_OK;
}

// The gradient arrays of `out`: the five leaves (where the form stores them) and the optional SH array
static int check_gradient_arrays(const char *fn, const gsplat_gradients *out, int l_max, bool leaves = true) {
  if (leaves) {
    GS_REQUIRE_DEV_IN(fn, out->grad_xyz); GS_REQUIRE_DEV_IN(fn, out->grad_rgb); GS_REQUIRE_DEV_IN(fn, out->grad_opacity);
    GS_REQUIRE_DEV_IN(fn, out->grad_scale); GS_REQUIRE_DEV_IN(fn, out->grad_quaternion);
    GS_REQUIRE_IN(fn, ((uintptr_t)out->grad_quaternion & 15) == 0, "grad_quaternion must be 16-byte aligned");
  }
  if (l_max > 0 && out->grad_sh) GS_REQUIRE_DEV_IN(fn, out->grad_sh);  // NULL: the caller rebuilds them (gsplat_optimizer_step_sh_factored)
  return GSPLAT_OK;
}

static const gsplat_gradients kNoArrays = {};  // split form: the twelve common columns go to `common`, nothing else is stored

// Everything the per-gaussian backward refuses, none of which needs a launch: a refused call leaves the caller's arrays
// as they were (gsplat_backward_gaussians_adam asks before its SH kernel steps anything)
static int check_backward_gaussians(const char *fn, const gsplat_context *c, const gsplat_gaussians *g,
                                    const gsplat_camera *cam, int l_max, const gsplat_gradients *out, const float *common,
                                    int first_gaussian, int end_gaussian, bool adam, int adam_mode, const float *grad_view,
                                    const float *grad_campos) {
  GS_REQUIRE_IN(fn, c && g && cam, "null argument struct");
  GS_REQUIRE_IN(fn, 0 <= first_gaussian && first_gaussian <= end_gaussian && end_gaussian <= g->num_gaussians, "bad gaussian range");
  GS_REQUIRE_IN(fn, c->have_forward && c->rows_ready, "gsplat_backward_render has not run for this forward pass");
  if (int rc = check_recorded_forward(fn, c, g, cam, l_max)) return rc;
  const bool cam_grad = grad_view != nullptr;  // gsplat_backward_gaussians_camera: whole range, plain form
  GS_REQUIRE_IN(fn, !(c->fwd_antialiased && adam),
                "the forward ran in anti-aliased mode: the Adam-inside backward steps the opacity before the covariance chain "
                "exists (use gsplat_backward_gaussians and the optimizer kernels)");
  GS_REQUIRE_IN(fn, !(c->fwd_antialiased && cam_grad), "the forward ran in anti-aliased mode: the camera gradient has no such form");
  GS_REQUIRE_IN(fn, !(c->fwd_filter3d && adam),
                "the forward ran with a 3D smoothing filter: the Adam-inside backward would step the filtered scale and "
                "opacity it differentiates (use gsplat_backward_gaussians and the optimizer kernels)");
  if (cam_grad) {
    GS_REQUIRE_DEV_IN(fn, grad_view); GS_REQUIRE_DEV_IN(fn, grad_campos);
    GS_REQUIRE_IN(fn, !adam && !common && first_gaussian == 0 && end_gaussian == g->num_gaussians, "internal: camera form");
  }
  if (!out) out = &kNoArrays;
  // (the Adam forms store only the arrays they are given; the camera form may be given none)
  const bool leaves = !common && !(adam && (out == &kNoArrays || adam_mode == 1)) && !(cam_grad && out == &kNoArrays);
  return check_gradient_arrays(fn, out, l_max, leaves);
}

static int backward_gaussians_impl(const char *fn, gsplat_context *c, const gsplat_gaussians *g, const gsplat_camera *cam,
                                   int l_max, const gsplat_gradients *out, float *common, float *uv_norm, int first_gaussian,
                                   int end_gaussian, void *stream, const gsplat_adam_fused *adam = nullptr, int adam_mode = 2,
                                   float *adam_dir = nullptr, float *grad_view = nullptr, float *grad_campos = nullptr) {
  int rc = check_backward_gaussians(fn, c, g, cam, l_max, out, common, first_gaussian, end_gaussian, adam != nullptr,
                                    adam_mode, grad_view, grad_campos);
  if (rc) return rc;
  const bool cam_grad = grad_view != nullptr;
  if (!out) out = &kNoArrays;
  hipStream_t st = (hipStream_t)stream;
  // 3D smoothing filter: the kernel recomputes from what the forward ran on -- the filtered scale and opacity, still in
  // the workspace -- and the chain rule to the raw ones follows it (below)
  const float *raw_scale = g->scale, *raw_opacity = g->opacity;
  gsplat_gaussians filtered;
  if (c->fwd_filter3d) {
    filtered = *g; filtered.scale = c->f3d_scale.as<float>(); filtered.opacity = c->f3d_opacity.as<float>();
    g = &filtered;
  }
  const int M = c->M, W = c->width, H = c->height;
  const float fx = cam->focal_x, fy = cam->focal_y;
  const float fov_x = (float)(2.0 * atan((double)W / (2.0 * (double)fx)));  // cuda/trainer.cu:992-995
  const float fov_y = (float)(2.0 * atan((double)H / (2.0 * (double)fy)));
  const float tan_fovx = tanf(fov_x * 0.5f), tan_fovy = tanf(fov_y * 0.5f);
  // a range of global indices holds at most that many visible gaussians (and never more than M); the kernel finds the
  // range's compacted slots in compact_to_global on the device (first_slot_not_below)
  const bool whole = first_gaussian == 0 && end_gaussian == g->num_gaussians;
  const int span = whole ? M : std::min(M, end_gaussian - first_gaussian);
  const int n_cam_rows = gs::div_up(span, 64);  // kCamGrad: one row of partial sums per wave
  if (cam_grad && span > 0 && (rc = c->cam_rows.reserve((size_t)n_cam_rows * 16 * sizeof(double), st))) return rc;
  if (span == 0) {
    if (cam_grad) {  // nothing visible: the camera gradient is zero, not what the buffers held
      GS_HIP(hipMemsetAsync(grad_view, 0, 12 * sizeof(float), st));
      GS_HIP(hipMemsetAsync(grad_campos, 0, 3 * sizeof(float), st));
    }
    return GSPLAT_OK;
  }
  c->mark(7, false, st);
  gs::PreprocessBwdArgs a = {};
  a.g = *g; a.view = cam->view; a.proj = cam->proj;
  a.M = M; a.c2g = c->c2g.as<int>(); a.xyz_c = c->xyz_c.as<float>(); a.rows = c->grad_rows.as<float4>();
  a.fx = fx; a.fy = fy; a.tan_fovx = tan_fovx; a.tan_fovy = tan_fovy;
  a.fwd_tan_fovx = c->tan_fovx; a.fwd_tan_fovy = c->tan_fovy;  // the recorded forward's (cuda/raster.cu:92-93)
  a.mh_dist = c->mh_dist;
  for (int k = 0; k < 3; ++k) a.campos[k] = cam->campos[k];
  a.width = W; a.height = H;
  a.out = *out; a.common = common; a.uv_norm = uv_norm;
  a.ranged = whole ? 0 : 1; a.first = first_gaussian; a.end = end_gaussian; a.span = span;
  if (adam) { a.adam = adam; a.adam_mode = adam_mode; a.adam_dir = adam_dir; }
  if (cam_grad) { a.cam_rows = c->cam_rows.as<double>(); a.grad_view = grad_view; a.grad_campos = grad_campos; }
  a.l_max = l_max; a.rows_depth = c->rows_depth; a.rows_abs = c->rows_abs;
  a.antialiased = c->fwd_antialiased;  // (plain form only: the Adam and camera forms were refused for such a forward above)
  // The forward's SH direction sums instead of the SH rows: the plain form and adam_mode 1 (the kernel's kAdam 1, which
  // steps nothing the sums were formed from before it has used them), and only the sums of the forward this call
  // differentiates, formed from the arrays and the camera this call was given.  (The degree needs no term of its own:
  // check_recorded_forward has refused any l_max but the recorded forward's, and the ticket says the sums are that forward's.)
  // An Adam form steps parameters in place, so whatever it read, the sums are nobody's afterwards.
  {
    const gsplat_context::DirSumsOf &of = c->dir_sums_of;
    const bool sums = c->dir_sums_on && !gs::no_dir_sums() && (!adam || adam_mode == 1) && !cam_grad && !a.antialiased && c->dir_sums.ptr != nullptr && of.ticket != 0 &&
                      of.ticket == c->fwd_ticket && of.xyz == g->xyz && of.rgb == g->rgb &&
                      of.sh == g->sh && of.view == cam->view && of.campos[0] == cam->campos[0] && of.campos[1] == cam->campos[1] &&
                      of.campos[2] == cam->campos[2];
    if (sums) a.dir_sums = c->dir_sums.as<float>();
    (sums ? c->n_dir_sums_backwards : c->n_dir_sums_fallbacks)++;
    if (adam) c->dir_sums_of.ticket = 0;
  }
  if ((rc = gs::launch_preprocess_bwd(a, st))) return rc;
  if (c->fwd_filter3d) {  // d/d (scale_eff, opacity_eff) -> d/d (scale, opacity), in place on the rows just written
    const int lo = whole ? 0 : first_gaussian, hi = whole ? 0 : end_gaussian;
    if (common)
      rc = gs::launch_filter3d_apply_bwd(raw_scale, raw_opacity, c->fwd_filter3d, c->c2g.as<int>(), M, common + 4, 12,
                                         common + 3, 12, true, lo, hi, span, st);
    else if (out->grad_scale && out->grad_opacity)
      rc = gs::launch_filter3d_apply_bwd(raw_scale, raw_opacity, c->fwd_filter3d, c->c2g.as<int>(), M, out->grad_scale, 3,
                                         out->grad_opacity, 1, false, lo, hi, span, st);
    if (rc) return rc;
  }
  c->mark(7, true, st);
  return GSPLAT_OK;
}

int gsplat_backward_gaussians(gsplat_context *c, const gsplat_gaussians *g, const gsplat_camera *cam, int l_max,
                              const gsplat_gradients *out, void *stream) {
  GS_REQUIRE(out != nullptr, "null argument struct");
  return backward_gaussians_impl(__func__, c, g, cam, l_max, out, nullptr, nullptr, 0, g ? g->num_gaussians : 0, stream);
}

int gsplat_backward_gaussians_range(gsplat_context *c, const gsplat_gaussians *g, const gsplat_camera *cam, int l_max,
                                    const gsplat_gradients *out, int first_gaussian, int end_gaussian, void *stream) {
  GS_REQUIRE(out != nullptr, "null argument struct");
  return backward_gaussians_impl(__func__, c, g, cam, l_max, out, nullptr, nullptr, first_gaussian, end_gaussian, stream);
}

int gsplat_backward_gaussians_split(gsplat_context *c, const gsplat_gaussians *g, const gsplat_camera *cam, int l_max,
                                    float *common, float *uv_norm, int first_gaussian, int end_gaussian, void *stream) {
  GS_REQUIRE_DEV(common);
  GS_REQUIRE(((uintptr_t)common & 15) == 0, "common must be 16-byte aligned");
  if (uv_norm) GS_REQUIRE_DEV(uv_norm);
  return backward_gaussians_impl(__func__, c, g, cam, l_max, nullptr, common, uv_norm, first_gaussian, end_gaussian, stream);
}

int gsplat_backward_gaussians_adam(gsplat_context *c, const gsplat_gaussians *g, const gsplat_camera *cam, int l_max,
                                   const gsplat_adam_fused *opt, const gsplat_gradients *out, void *stream) {
  GS_REQUIRE(opt != nullptr && g != nullptr, "null argument struct");
  for (int k = 0; k < 6; ++k) {
    if (k == 2 && l_max == 0) continue;  // no coefficients beyond band 0
    GS_REQUIRE_DEV(opt->exp_avg[k]); GS_REQUIRE_DEV(opt->exp_avg_sq[k]);
  }
  GS_REQUIRE(((uintptr_t)opt->exp_avg[5] & 15) == 0 && ((uintptr_t)opt->exp_avg_sq[5] & 15) == 0,
             "the quaternion moments must be 16-byte aligned");
  if (opt->uv_grad_accum) GS_REQUIRE_DEV(opt->uv_grad_accum);
  if (opt->grad_accum_dur) GS_REQUIRE_DEV(opt->grad_accum_dur);
  GS_REQUIRE(opt->mode >= 0 && opt->mode <= 2,
             "mode: 0 all six groups in one kernel, 1 SH and position left to the optimizer kernels, 2 the SH group in a kernel of its own in front");
  if (opt->mode == 1) {
    GS_REQUIRE(out != nullptr, "mode 1 hands grad_xyz and grad_precompute_rgb to the optimizer kernels: `out` is needed");
    GS_REQUIRE_DEV(out->grad_xyz);
    if (l_max > 0) GS_REQUIRE_DEV(out->grad_precompute_rgb);
  }
  const int adam_mode = opt->mode == 1 ? 1 : opt->mode == 2 ? 3 : 2;
  // everything the per-gaussian backward below could refuse, BEFORE sh_adam_dir_kernel steps the SH group in place
  int rc = check_backward_gaussians(__func__, c, g, cam, l_max, out, nullptr, 0, g->num_gaussians, true, adam_mode, nullptr, nullptr);
  if (rc) return rc;
  float *dir = nullptr;
  if (opt->mode == 2 && l_max > 0 && c->M > 0) {
    // the SH rows are read ONCE, by sh_adam_dir_kernel: their Adam step and sh_bwd's sums over them; the per-gaussian
    // backward behind it (kAdam 3) takes the position gradient through the view direction from c->dir_grad
    hipStream_t st = (hipStream_t)stream;
    if ((rc = c->dir_grad.reserve((size_t)c->M * 3 * sizeof(float), st))) return rc;
    dir = c->dir_grad.as<float>();
    gs::ShAdamDirArgs a = {};
    a.M = c->M; a.c2g = c->c2g.as<int>();
    a.sh = const_cast<float *>(g->sh); a.m = opt->exp_avg[2]; a.v = opt->exp_avg_sq[2];
    a.lr = opt->lr[2]; a.b1 = opt->b1; a.b2 = opt->b2; a.eps = opt->eps; a.bias1 = opt->bias1; a.bias2 = opt->bias2;
    a.xyz = g->xyz; a.band0 = g->rgb;
    for (int k = 0; k < 3; ++k) a.campos[k] = cam->campos[k];
    a.rows = c->grad_rows.as<float4>(); a.dir_out = dir;
    a.l_max = l_max;
    if ((rc = gs::launch_sh_adam_dir(a, st))) return rc;
  }
  return backward_gaussians_impl(__func__, c, g, cam, l_max, out, nullptr, nullptr, 0, g->num_gaussians, stream, opt, adam_mode, dir);
}

int gsplat_backward_gaussians_camera(gsplat_context *c, const gsplat_gaussians *g, const gsplat_camera *cam, int l_max,
                                     const gsplat_gradients *out, float *grad_view, float *grad_campos, void *stream) {
  GS_REQUIRE_DEV(grad_view); GS_REQUIRE_DEV(grad_campos);
  return backward_gaussians_impl(__func__, c, g, cam, l_max, out, nullptr, nullptr, 0, g ? g->num_gaussians : 0, stream,
                                 nullptr, 2, nullptr, grad_view, grad_campos);
}

// gsplat_backward_pass*: every check of the two halves before the first launch, then the halves.  `camera`: the form
// that also returns the pose gradient and may be given no `out`.
static int backward_pass(const char *fn, gsplat_context *c, const gsplat_gaussians *g, const gsplat_camera *cam,
                         const float *grad_image, const float *grad_depth, const float *grad_alpha, float bg_color,
                         int l_max, const gsplat_gradients *out, bool camera, float *grad_view, float *grad_campos,
                         void *stream, const float *grad_depth2 = nullptr) {
  GS_REQUIRE_IN(fn, c && g && cam && (out || camera), "null argument struct");
  int rc = check_recorded_forward(fn, c, g, cam, l_max);
  if (rc) return rc;
  if (camera) {
    GS_REQUIRE_DEV_IN(fn, grad_view); GS_REQUIRE_DEV_IN(fn, grad_campos);
    GS_REQUIRE_IN(fn, !c->fwd_antialiased, "the forward ran in anti-aliased mode: the camera gradient has no such form");
  }
  if (out && (rc = check_gradient_arrays(fn, out, l_max))) return rc;
  // (the compositing half checks its own arguments before its first launch)
  rc = gsplat_backward_render_depth2(c, grad_image, grad_depth, grad_alpha, grad_depth2, bg_color, /*rgb_global=*/nullptr,
                                     /*common=*/nullptr, /*uv_norm=*/nullptr, stream);
  if (rc) return rc;
  return backward_gaussians_impl(fn, c, g, cam, l_max, out, nullptr, nullptr, 0, g->num_gaussians, stream, nullptr, 2,
                                 nullptr, grad_view, grad_campos);
}

int gsplat_backward_pass(gsplat_context *c, const gsplat_gaussians *g, const gsplat_camera *cam, const float *grad_image,
                         float bg_color, int l_max, const gsplat_gradients *out, void *stream) {  // (the depth form with two null maps: the plain backward, exactly)
  return backward_pass(__func__, c, g, cam, grad_image, nullptr, nullptr, bg_color, l_max, out, false, nullptr, nullptr, stream);
}

int gsplat_backward_pass_depth(gsplat_context *c, const gsplat_gaussians *g, const gsplat_camera *cam,
                               const float *grad_image, const float *grad_depth, const float *grad_alpha, float bg_color,
                               int l_max, const gsplat_gradients *out, void *stream) {
  return backward_pass(__func__, c, g, cam, grad_image, grad_depth, grad_alpha, bg_color, l_max, out, false, nullptr, nullptr, stream);
}

int gsplat_backward_pass_depth2(gsplat_context *c, const gsplat_gaussians *g, const gsplat_camera *cam,
                                const float *grad_image, const float *grad_depth, const float *grad_alpha,
                                const float *grad_depth2, float bg_color, int l_max, const gsplat_gradients *out, void *stream) {
  return backward_pass(__func__, c, g, cam, grad_image, grad_depth, grad_alpha, bg_color, l_max, out, false, nullptr, nullptr, stream,
                       grad_depth2);
}

int gsplat_backward_pass_camera(gsplat_context *c, const gsplat_gaussians *g, const gsplat_camera *cam,
                                const float *grad_image, const float *grad_depth, const float *grad_alpha, float bg_color,
                                int l_max, const gsplat_gradients *out, float *grad_view, float *grad_campos, void *stream) {
  return backward_pass(__func__, c, g, cam, grad_image, grad_depth, grad_alpha, bg_color, l_max, out, true, grad_view, grad_campos, stream);
}

}  // extern "C"
