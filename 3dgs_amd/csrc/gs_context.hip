// gs_context.hip -- the life cycle of a gsplat_context (gs_context.h) and everything that only sets or reads its state:
// create / destroy / bytes, the mode setters, counters, per-stage timing, the depth map, the last compaction, the hand-over
// of the forward's outputs and the contribution statistics; and the room of the instance buffers (instance_room,
// reserve_instances), which the forward in gs_fused.hip grows.  No kernel lives here.
#include <cstdlib>
#include <new>
#include <vector>

#include "gs_context.h"
#include "gs_launch.h"

namespace gs {

// ---- the environment switches (gs_context.h): one reader per kind of value, one function-local static per switch ----
static bool env_is(const char *name, char c) { const char *e = getenv(name); return e && e[0] == c; }
static int env_digit(const char *name, int lo, int hi, int otherwise) {  // the first character as a digit lo..hi
  const char *e = getenv(name);
  return e && e[0] >= '0' + lo && e[0] <= '0' + hi ? e[0] - '0' : otherwise;
}
static double env_number(const char *name, double otherwise) { const char *e = getenv(name); return e && e[0] ? atof(e) : otherwise; }

int pre_split_default() { static const int v = env_digit("GSPLAT_PRE_SPLIT", 0, 2, 0); return v; }
bool pre_join_late() { static const bool v = env_is("GSPLAT_PRE_JOIN", 'l'); return v; }
bool no_tile_order() { static const bool v = env_is("GSPLAT_NO_TILE_ORDER", '1'); return v; }
bool no_compact_lists() { static const bool v = env_is("GSPLAT_NO_COMPACT_LISTS", '1'); return v; }
bool no_segments() { static const bool v = env_is("GSPLAT_NO_SEGMENTS", '1'); return v; }
bool no_fwd_segments() { static const bool v = env_is("GSPLAT_NO_FWD_SEGMENTS", '1'); return v; }
double fwd_segments_gate() { static const double v = env_number("GSPLAT_FWD_SEGMENTS_GATE", 3.0); return v; }
bool no_dir_sums() { static const bool v = env_is("GSPLAT_NO_DIR_SUMS", '1'); return v; }

// Room of the instance buffers, in INSTANCES: the smallest element count of the per-instance arrays, minus the one spare
// slot every user keeps.  Each array is a DeviceBuffer grown by `want + want / 4 + 256` BYTES, so arrays of different
// element size end up with different element counts for the same S (8-byte payloads: 32 entries of slack, 4-byte keys:
// 64, 2-byte masks: 128) -- a bound taken from one array alone is not a bound for the others.  Until r05 the radix
// route bounded its speculative tile_emit_payload_kernel by keys_a's count only, 31 entries more than pay_a holds: a
// forward whose instances outgrew the room wrote 248 bytes past the end of pay_a (test_instance_buffers_grow's radix
// case: a 12 266-byte allocation that ends 22 bytes before its page does; whether the next page is mapped depends on
// what the allocator placed there -- the unexplained abort of r04's suite).
size_t instance_room(const gsplat_context *c) {
  size_t room = c->keys_a.bytes / sizeof(unsigned int);
  room = std::min(room, c->keys_b.bytes / sizeof(unsigned int));
  room = std::min(room, c->pay_a.bytes / sizeof(unsigned long long));
  room = std::min(room, c->pay_b.bytes / sizeof(unsigned long long));
  room = std::min(room, c->sorted.bytes / sizeof(int));
  room = std::min(room, c->blockmasks.bytes / sizeof(unsigned short));
  room = std::min(room, c->ids_c.bytes / sizeof(int));
  room = std::min(room, c->masks_c.bytes / sizeof(unsigned short));
  return room;
}

int reserve_instances(gsplat_context *c, size_t S, int num_tiles, hipStream_t st) {
  int rc;
  const void *pay_before = c->pay_a.ptr, *sorted_before = c->sorted.ptr;
  if ((rc = c->keys_a.reserve((S + 1) * sizeof(unsigned int)))) return rc;
  if ((rc = c->keys_b.reserve((S + 1) * sizeof(unsigned int)))) return rc;
  if ((rc = c->pay_a.reserve((S + 1) * sizeof(unsigned long long)))) return rc;
  if ((rc = c->pay_b.reserve((S + 1) * sizeof(unsigned long long)))) return rc;
  if ((rc = c->sorted.reserve((S + 1) * sizeof(int)))) return rc;
  // Fresh instance buffers start as zeros.  The sparse forward queues its sorts and render_fwd before the host has
  // seen S; when S outgrows the room those kernels run on truncated lists whose slots may not have been written by
  // this forward -- whatever they hold must still be a valid gaussian id (0, or one of an earlier forward).
  // The fill goes on the CALLER's stream: on the NULL stream nothing would order it against the placement and the sorts
  // that a non-blocking stream (a torch side stream) runs right behind it, and the zeros could land on top of them.
  if (c->pay_a.ptr != pay_before) GS_HIP(hipMemsetAsync(c->pay_a.ptr, 0, c->pay_a.bytes, st));
  if (c->sorted.ptr != sorted_before) GS_HIP(hipMemsetAsync(c->sorted.ptr, 0, c->sorted.bytes, st));
  if ((rc = c->blockmasks.reserve((S + 1) * sizeof(unsigned short)))) return rc;
  // (the compact lists need no fill: the backward reads only the positions the forward it follows has written)
  if ((rc = c->ids_c.reserve((S + 1) * sizeof(int)))) return rc;
  if ((rc = c->masks_c.reserve((S + 1) * sizeof(unsigned short)))) return rc;
  if ((rc = c->temp.reserve(gs::binning_temp_bytes((size_t)c->max_gaussians, S ? S : 1, num_tiles)))) return rc;
  return GSPLAT_OK;
}

// the forward this context recorded (lists_ready), for the kernels that walk it again
static ReplayArgs recorded_forward(gsplat_context *c) {
  ReplayArgs a = {};
  a.recs = c->recs.as<float4>();
  a.sorted = c->sorted.as<int>(); a.ranges = c->ranges.as<int>();
  a.n_px = c->n_px.as<int>(); a.T_px = c->T_px.as<float>();
  a.c2g = c->c2g.as<int>();
  a.width = c->width; a.height = c->height;
  return a;
}

}  // namespace gs

extern "C" {

int gsplat_context_create(gsplat_context **out, int max_gaussians, int max_width, int max_height) {
  GS_REQUIRE(out != nullptr, "out is null");
  GS_REQUIRE(max_gaussians > 0 && max_width > 0 && max_height > 0, "capacities must be positive");
  gsplat_context *c = new (std::nothrow) gsplat_context();
  GS_REQUIRE(c != nullptr, "out of host memory");
  c->max_gaussians = max_gaussians; c->max_width = max_width; c->max_height = max_height;
  const size_t N = (size_t)max_gaussians, P = (size_t)max_width * max_height;
  const size_t T = (size_t)((max_width + 15) / 16) * ((max_height + 15) / 16);
  int rc = GSPLAT_OK;
  {
    gs::DeviceBuffer *outs[13];
    c->forward_outputs(outs);
    for (gs::DeviceBuffer *b : outs) b->pooled = true;
  }
  auto R = [&](gs::DeviceBuffer &b, size_t bytes) { if (!rc) rc = b.reserve(bytes); };
  R(c->mask, N + 16); R(c->counters, 512 + gs::kBinBlocks * 4 + 64); R(c->rank, (N + 1) * 4); R(c->xyz_c_all, N * 12); R(c->uv_all, N * 8);
  R(c->c2g, N * 4); R(c->xyz_c, N * 12); R(c->uv, N * 8); R(c->sigma, N * 24); R(c->conic, N * 12); R(c->J, N * 24);
  R(c->rgb, N * 12); R(c->radius, N * 16); R(c->recs, N * 48); R(c->counts, (N + 1) * 4); R(c->offsets, (N + 1) * 4);
  R(c->grad_rows, N * 64); R(c->hitmask, N * 8);
  R(c->ranges, (T + 1) * 4); R(c->image, P * 12); R(c->T_px, P * 4); R(c->n_px, P * 4);
  R(c->tile_tops, (T + 8) * 4); R(c->tile_order, (T + 8) * 4);
  R(c->n_c_px, P * 4); R(c->tile_useful, (T + 8) * 4);
  if (!rc) {
    const size_t sb1 = gs::scan_counts_temp_bytes(N);
    const size_t sb2 = gs::binning_temp_bytes(N, 4 * N, (int)T);
    rc = c->temp.reserve(sb1 > sb2 ? sb1 : sb2);
  }
  if (!rc && hipMemsetAsync(c->counters.ptr, 0, c->counters.bytes, (hipStream_t)0) != hipSuccess) rc = GSPLAT_ERR_HIP;
  if (!rc) rc = gs::reserve_instances(c, 4 * N, (int)T, (hipStream_t)0);
  if (!rc && hipStreamSynchronize((hipStream_t)0) != hipSuccess) {  // the fills above: done before any stream uses the context
    gs::set_error("gsplat_context_create: hipStreamSynchronize failed");
    rc = GSPLAT_ERR_HIP;
  }
  if (!rc) {
    void *h = nullptr, *d = nullptr;
    if (hipHostMalloc(&h, 256, hipHostMallocMapped | hipHostMallocCoherent) != hipSuccess ||
        hipHostGetDevicePointer(&d, h, 0) != hipSuccess) {
      gs::set_error("gsplat_context_create: could not map the count record");
      rc = GSPLAT_ERR_HIP;
    } else {
      memset(h, 0, 256);  // words 0..4: the forward's record; 8..15: two slots of four tagged figures (queue_sparse_tail)
      c->h_pub = (volatile unsigned long long *)h;
      c->d_pub = (unsigned long long *)d;
    }
  }
  if (!rc && hipHostMalloc((void **)&c->h_words, 1024, hipHostMallocDefault) != hipSuccess) {
    gs::set_error("gsplat_context_create: hipHostMalloc failed");
    rc = GSPLAT_ERR_HIP;
  }
  if (rc) { c->release(); delete c; return rc; }
  *out = c;
  return GSPLAT_OK;
}

int gsplat_context_destroy(gsplat_context *ctx) {
  if (!ctx) return GSPLAT_OK;
  (void)hipDeviceSynchronize();
  ctx->release();
  delete ctx;
  // the context's pooled output arrays went back to the pool's idle lists.  r06: they stay there for the next context /
  // the shim's vectors of this device unless more than a gigabyte is idle on it (gsplat_pool_trim) -- r05 called the
  // process-wide gsplat_pool_release here, which synchronised every device and emptied the caches of live peers
  (void)gsplat_pool_trim((size_t)1 << 30);
  return GSPLAT_OK;
}

size_t gsplat_context_bytes(const gsplat_context *ctx) { return ctx ? ctx->bytes() : 0; }

int gsplat_context_last_compaction(gsplat_context *c, const unsigned char **mask, const int **slots,
                                   const int **compact_to_global, int *num_gaussians, int *num_culled) {
  GS_REQUIRE(c != nullptr, "null context");
  const bool have = c->n_forwards > 0 && c->last_mask != nullptr;
  if (mask) *mask = have ? c->last_mask : nullptr;
  if (slots) *slots = have ? c->rank.as<int>() : nullptr;
  if (compact_to_global) *compact_to_global = have ? c->c2g.as<int>() : nullptr;
  if (num_gaussians) *num_gaussians = have ? c->N : 0;
  if (num_culled) *num_culled = have ? c->M : 0;
  return GSPLAT_OK;
}

int gsplat_context_detach_forward_outputs(gsplat_context *c) {
  GS_REQUIRE(c != nullptr, "null context");
  GS_REQUIRE(c->n_forwards > 0 && c->mask.ptr != nullptr, "no forward whose outputs could be handed over");
  GS_REQUIRE(!c->lean && !c->render_only, "a lean / render-only forward does not fill all ForwardPassData arrays");
  gs::DeviceBuffer *outs[13];
  c->forward_outputs(outs);
  for (gs::DeviceBuffer *b : outs) (void)b->detach();  // the caller owns the blocks now (gsplat_pool_free)
  c->have_forward = false;  // the fused backward would read arrays this context no longer has
  c->lists_ready = false;
  c->rows_ready = false;
  return GSPLAT_OK;
}

int gsplat_context_set_depth(gsplat_context *c, int enabled) {
  GS_REQUIRE(c != nullptr, "null context");
  c->depth = enabled != 0;
  c->depth_inverse = c->depth_moment = false;  // (the options are gsplat_context_set_depth_mode's)
  return GSPLAT_OK;
}

int gsplat_context_set_depth_mode(gsplat_context *c, int inverse, int moment) {
  GS_REQUIRE(c != nullptr, "null context");
  c->depth = true;
  c->depth_inverse = inverse != 0;
  c->depth_moment = moment != 0;
  return GSPLAT_OK;
}

int gsplat_context_set_antialiased(gsplat_context *c, int enabled) {
  GS_REQUIRE(c != nullptr, "null context");
  c->antialiased = enabled != 0;  // (read by the next forward; a backward follows the forward it belongs to)
  return GSPLAT_OK;
}

int gsplat_context_set_filter3d(gsplat_context *c, const float *filter3d) {
  GS_REQUIRE(c != nullptr, "null context");
  if (filter3d) GS_REQUIRE_DEV(filter3d);
  c->filter3d = filter3d;  // (read by the next forward; a backward follows the forward it belongs to)
  return GSPLAT_OK;
}

int gsplat_context_set_compact_lists(gsplat_context *c, int enabled) {
  GS_REQUIRE(c != nullptr, "null context");
  c->compact_lists = enabled != 0;  // (read by the next forward; a backward follows the forward it belongs to)
  return GSPLAT_OK;
}

int gsplat_context_set_dir_sums(gsplat_context *c, int enabled) {
  GS_REQUIRE(c != nullptr, "null context");
  c->dir_sums_on = enabled != 0;  // (read by the next forward; a backward follows the forward it belongs to)
  return GSPLAT_OK;
}

int gsplat_context_set_absgrad(gsplat_context *c, int enabled) {
  GS_REQUIRE(c != nullptr, "null context");
  c->absgrad = enabled != 0;  // (read by the next compositing backward; the forward has no part in it)
  return GSPLAT_OK;
}

int gsplat_context_accumulate_contributions(gsplat_context *c, int num_gaussians, float *weight_sum, float *weight_max,
                                            int *pixels, void *stream) {
  // (every check before the launch: a refused call leaves the caller's arrays as they were)
  GS_REQUIRE(c != nullptr, "null context");
  GS_REQUIRE(weight_sum || weight_max || pixels, "no statistic asked for: weight_sum, weight_max and pixels are all NULL");
  GS_REQUIRE(c->lists_ready, "no forward pass recorded in this context");
  GS_REQUIRE(num_gaussians == c->N, "does not match the recorded forward");
  if (weight_sum) GS_REQUIRE_DEV(weight_sum);
  if (weight_max) GS_REQUIRE_DEV(weight_max);
  if (pixels) GS_REQUIRE_DEV(pixels);
  return gs::launch_contributions(gs::recorded_forward(c), weight_sum, weight_max, pixels, (hipStream_t)stream);
}

int gsplat_context_median_depth(gsplat_context *c, int num_gaussians, float threshold, float *depth, int *index,
                                void *stream) {
  // (every check before the launch: a refused call leaves the caller's arrays as they were)
  GS_REQUIRE(c != nullptr, "null context");
  GS_REQUIRE(c->lists_ready, "no forward pass recorded in this context");
  GS_REQUIRE(num_gaussians == c->N, "does not match the recorded forward");
  GS_REQUIRE(std::isfinite(threshold) && threshold > 0.0f && threshold < 1.0f, "threshold must lie in (0, 1)");
  GS_REQUIRE(depth != nullptr && gs::check_device_ptr(depth, "depth", __func__) == GSPLAT_OK,
             "depth must be a device pointer");
  GS_REQUIRE(index == nullptr || gs::check_device_ptr(index, "index", __func__) == GSPLAT_OK,
             "index must be a device pointer or NULL");
  return gs::launch_median_depth(gs::recorded_forward(c), c->xyz_c.as<float>(), threshold, depth, index,
                                 (hipStream_t)stream);
}

int gsplat_context_render_features(gsplat_context *c, int num_gaussians, int channels, const float *features, float *out,
                                   void *stream) {
  // (every check before the launch: a refused call leaves the caller's arrays as they were)
  GS_REQUIRE(c != nullptr, "null context");
  GS_REQUIRE(c->lists_ready, "no forward pass recorded in this context");
  GS_REQUIRE(num_gaussians == c->N, "does not match the recorded forward");
  GS_REQUIRE(channels >= 1 && channels <= 512, "channels must be 1 .. 512");
  GS_REQUIRE_DEV(features);
  GS_REQUIRE_DEV(out);
  return gs::launch_features_fwd(gs::recorded_forward(c), channels, features, out, (hipStream_t)stream);
}

int gsplat_context_lift_features(gsplat_context *c, int num_gaussians, int channels, const float *map, float *lifted,
                                 void *stream) {
  GS_REQUIRE(c != nullptr, "null context");
  GS_REQUIRE(c->lists_ready, "no forward pass recorded in this context");
  GS_REQUIRE(num_gaussians == c->N, "does not match the recorded forward");
  GS_REQUIRE(channels >= 1 && channels <= 512, "channels must be 1 .. 512");
  GS_REQUIRE_DEV(map);
  GS_REQUIRE_DEV(lifted);
  return gs::launch_features_lift(gs::recorded_forward(c), channels, map, lifted, (hipStream_t)stream);
}

int gsplat_context_features_backward(gsplat_context *c, int num_gaussians, int channels, const float *features,
                                     const float *grad_map, void *stream) {
  // (every check before the launch: a refused call leaves the gradient rows and the caller's arrays as they were; every
  // refusal of this entry point is GSPLAT_ERR_INVALID_ARG, a null or non-device pointer included)
  GS_REQUIRE(c != nullptr, "null context");
  GS_REQUIRE(c->lists_ready, "no forward pass recorded in this context");
  GS_REQUIRE(c->have_forward && c->rows_ready,
             "gsplat_backward_render has not run for this forward pass: the feature term is added to its gradient rows");
  GS_REQUIRE(num_gaussians == c->N, "does not match the recorded forward");
  GS_REQUIRE(channels >= 1 && channels <= 512, "channels must be 1 .. 512");
  GS_REQUIRE(features != nullptr && gs::check_device_ptr(features, "features", __func__) == GSPLAT_OK,
             "features must be a device pointer");
  GS_REQUIRE(grad_map != nullptr && gs::check_device_ptr(grad_map, "grad_map", __func__) == GSPLAT_OK,
             "grad_map must be a device pointer");
  return gs::launch_features_bwd(gs::recorded_forward(c), channels, features, grad_map, c->grad_rows.as<float>(),
                                 (hipStream_t)stream);
}

int gsplat_context_depth_map(gsplat_context *c, const float **depth) {
  GS_REQUIRE(c && depth, "null argument");
  *depth = nullptr;
  GS_REQUIRE(c->n_forwards > 0 && c->depth_ready, "the last forward did not render depth (gsplat_context_set_depth)");
  *depth = c->depth_map.as<float>();
  return GSPLAT_OK;
}

int gsplat_context_depth_moment_map(gsplat_context *c, const float **q) {
  GS_REQUIRE(c && q, "null argument");
  *q = nullptr;
  GS_REQUIRE(c->n_forwards > 0 && c->depth_ready && c->depth_moment_ready,
             "the last forward did not render the second moment (gsplat_context_set_depth_mode)");
  *q = c->depth2_map.as<float>();
  return GSPLAT_OK;
}

int gsplat_context_set_binning_route(gsplat_context *c, int route) {
  GS_REQUIRE(c != nullptr, "null context");
  GS_REQUIRE(route >= 0 && route <= 2, "route: 0 auto, 1 counting sort, 2 radix sorts");
  c->forced_route = route;
  return GSPLAT_OK;
}

int gsplat_context_set_segment_options(gsplat_context *c, int poll_budget, int thin_layer_blocks, float gate) {
  GS_REQUIRE(c != nullptr, "null context");
  if (poll_budget >= 0) c->fseg_poll_budget = poll_budget > 0 ? poll_budget : 1;
  if (thin_layer_blocks >= 0) c->fseg_thin_layer = thin_layer_blocks;
  if (gate >= 0.0f) c->fseg_gate = gate;
  return GSPLAT_OK;
}

int gsplat_context_set_timing_stages(gsplat_context *c, unsigned int stage_mask) {
  GS_REQUIRE(c != nullptr, "null context");
  if (stage_mask && !c->ev[0][0]) {
    for (int a = 0; a < gsplat_context::kSlots; ++a)
      for (int b = 0; b < 2 * gsplat_context::kStages; ++b) GS_HIP(hipEventCreate(&c->ev[a][b]));
  }
  GS_HIP(hipDeviceSynchronize());
  for (int a = 0; a < gsplat_context::kSlots; ++a) c->harvest(a);
  for (int k = 0; k < gsplat_context::kStages; ++k) { c->stage_ms[k] = 0; c->stage_n[k] = 0; }
  c->timing = stage_mask & ((1u << gsplat_context::kStages) - 1u);
  return GSPLAT_OK;
}

int gsplat_context_get_counters(gsplat_context *c, long long *out, int n) {
  GS_REQUIRE(c && out && n >= 0, "null argument");
  // (reporting only: the freshest pair of figures either slot holds -- the forward's decisions use gs::take_figures)
  long long fmax = c->fig.max, fsum = c->fig.sum;
  unsigned int best = 0;
  for (int sl = 0; sl < 2; ++sl) {
    const unsigned long long w0 = __atomic_load_n(&c->h_pub[8 + 4 * sl], __ATOMIC_RELAXED);
    const unsigned long long w1 = __atomic_load_n(&c->h_pub[9 + 4 * sl], __ATOMIC_RELAXED);
    const unsigned int tag = (unsigned int)(w0 >> 32);
    if (tag != 0 && tag == (unsigned int)(w1 >> 32) && tag >= best && tag <= (unsigned int)(c->ticket & 0xFFFFFFFFull)) {
      best = tag; fmax = (long long)(int)(unsigned int)w0; fsum = (long long)(int)(unsigned int)w1;
    }
  }
  int fallbacks = 0;  // (a blocking 4-byte copy: this is a diagnostic call)
  if (n > 9 && c->counters.ptr) GS_HIP(hipMemcpy(&fallbacks, c->fseg_fallbacks(), sizeof(int), hipMemcpyDeviceToHost));
  // out[11]: the tiles' useful totals of the last forward that wrote compact lists, summed on request (a blocking copy of
  // one int per tile behind everything queued on the device: a diagnostic call)
  long long useful = 0;
  if (n > 11 && c->compact_written && c->have_forward) {
    const size_t tiles = (size_t)((c->width + 15) / 16) * ((c->height + 15) / 16);
    std::vector<int> h(tiles);
    GS_HIP(hipDeviceSynchronize());
    GS_HIP(hipMemcpy(h.data(), c->tile_useful.ptr, tiles * sizeof(int), hipMemcpyDeviceToHost));
    for (int u : h) useful += u;
  }
  const long long v[14] = {c->n_forwards, c->n_tail_redone, c->n_compact_walks, c->n_instance_growths, c->n_ordered_backwards,
                           (long long)c->n_segmented_backwards, (long long)c->n_segmented_forwards, fmax, fsum, fallbacks,
                           c->n_compact_backwards, useful, c->n_dir_sums_backwards, c->n_dir_sums_fallbacks};
  for (int k = 0; k < n && k < 14; ++k) out[k] = v[k];
  return 14;
}

int gsplat_context_set_render_only(gsplat_context *c, int enabled) {
  GS_REQUIRE(c != nullptr, "null context");
  c->render_only = enabled != 0;
  if (c->render_only) c->have_forward = false;
  return GSPLAT_OK;
}

int gsplat_context_set_preprocess_split(gsplat_context *c, int mode) {
  GS_REQUIRE(c != nullptr, "null context");
  GS_REQUIRE(mode >= 0 && mode <= 2, "mode: 0 one kernel, 1 two kernels in sequence, 2 two kernels side by side");
  c->pre_split = mode;
  return GSPLAT_OK;
}

int gsplat_context_set_lean_forward(gsplat_context *c, int enabled) {
  GS_REQUIRE(c != nullptr, "null context");
  c->lean = enabled != 0;
  return GSPLAT_OK;
}

int gsplat_context_set_timing(gsplat_context *c, int enabled) {
  return gsplat_context_set_timing_stages(c, enabled ? ~0u : 0u);
}

int gsplat_context_get_timing(gsplat_context *c, double *stage_ms_sum, long long *stage_count, int max_stages) {
  GS_REQUIRE(c && stage_ms_sum && stage_count, "null argument");
  GS_HIP(hipDeviceSynchronize());
  for (int a = 0; a < gsplat_context::kSlots; ++a) c->harvest(a);
  for (int k = 0; k < max_stages && k < gsplat_context::kStages; ++k) {
    stage_ms_sum[k] = c->stage_ms[k];
    stage_count[k] = c->stage_n[k];
  }
  return gsplat_context::kStages;
}

}  // extern "C"
