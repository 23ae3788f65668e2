// gs_forward_plan.h -- the decisions gsplat_rasterize_image (gs_fused.hip) takes on the host, as functions of plain
// numbers: which walk the per-gaussian kernel does, which sort kernels a tile list needs, whether a tail queued before
// the counts were known has to be redone, whether tile order and the forward split pay, how much segment room to
// reserve, which published figures may be trusted, and how the forward's host record is laid out.  Plain C++17 with no
// HIP include, so that a host compiler builds it alone (tests/cpp/forward_plan_test.cpp); the launches, the atomic
// loads and everything that touches a context (gs_context.h) stay in gs_fused.hip.
#pragma once
#include <algorithm>
#include <cstddef>

#ifdef __HIPCC__
#define GS_PLAN_HD __host__ __device__
#else
#define GS_PLAN_HD
#endif

namespace gs {

// The forward's host record: pinned, mapped host memory the GPU writes and the host polls.  Five 64-bit words, each
// {value << 32 | low half of the forward's ticket}: M, S, candidate pairs (low, high), longest tile list.  A word is
// one aligned 8-byte store, so it cannot tear, and the host takes the record when all five carry its ticket -- no
// ordering between the stores is needed, hence no __threadfence_system() (a system-scope release writes back the
// XCD's whole L2: several microseconds on the GPU's critical path, behind kernels that left megabytes dirty).
constexpr int kRecordWords = 5;
GS_PLAN_HD inline unsigned long long record_word(unsigned int value, unsigned long long ticket) {
  return ((unsigned long long)value << 32) | (ticket & 0xFFFFFFFFull);
}
// `w`: the five words as the host loaded them (the loads and the acquire fence are the caller's)
inline bool record_arrived(const unsigned long long w[kRecordWords], unsigned long long ticket) {
  for (int k = 0; k < kRecordWords; ++k)
    if ((w[k] & 0xFFFFFFFFull) != (ticket & 0xFFFFFFFFull)) return false;
  return true;
}
struct ForwardRecord {
  int M;                     // gaussians in view
  size_t S;                  // tile instances
  unsigned long long pairs;  // coarse candidate pairs (reporting only)
  long long longest;         // longest tile list (the counting-sort route publishes it; the radix route's word is void)
};
inline ForwardRecord decode_record(const unsigned long long w[kRecordWords]) {
  return {(int)(unsigned int)(w[0] >> 32), (size_t)(w[1] >> 32), (w[2] >> 32) | (w[3] & 0xFFFFFFFF00000000ull),
          (long long)(w[4] >> 32)};
}

// A view that culled a fifth of the scene or more last time gets the compacted walk in preprocess_kernel (the previous
// forward of the context decides: views of a training run look alike; the first call walks all indices).
inline bool compact_walk(int prev_N, int prev_M, int N) {
  return prev_N == N && prev_M > 0 && ((long long)prev_M * 5 < (long long)N * 4);
}

// Which of the workgroup sort kernels a list of that length needs.  Class 0: no list beyond the wave kernel's 1024
// entries and every depth key an ordinary positive float (keys_ok) -- the hand-over kernel is not queued at all
// (gs_binning.hip sort_tiles_by_depth).
inline int sort_class(long long longest, bool keys_ok) {
  return longest > 8 * 1024 ? 4 : longest > 4 * 1024 ? 3 : longest > 2 * 1024 ? 2 : (longest > 1024 || !keys_ok) ? 1 : 0;
}
// The longest list the tail queued before the counts are known is prepared for: half again the last forward's, or -1
// (unknown: every kernel).
inline long long speculative_longest(long long last_longest) {
  return last_longest >= 0 ? last_longest + last_longest / 2 + 64 : -1;
}
// Sparse route: nothing behind the counts needs them on the HOST -- the placement only needs room for its writes, the
// per-tile sorts read `ranges` on the device, the compositing nothing at all.  So scatter, sorts and render_fwd are
// queued bounded by the buffers' capacity and the host sleeps on the read-back while they run (r01 launched them after
// the wake-up: the GPU idled for the round trip, ~13 us per forward).  Afterwards the record is checked: the queued tail
// is redone, from the placement on, when its instances outgrew the room it was bounded by or the longest list needs a
// sort kernel that was not queued (results are unaffected: every launch overwrites).
inline bool tail_needs_redo(size_t S, size_t spec_cap, long long spec_hint, long long longest, bool keys_ok) {
  const bool fits = S <= spec_cap;
  return !fits || !(spec_hint < 0 || sort_class(longest, keys_ok) <= sort_class(spec_hint, keys_ok));
}

// Heaviest-first tiles for the backward only where the tiles differ enough in work to pay for it -- the last forward's
// longest list against three times its average: the order breaks up the XCD runs' spatial adjacency (neighbouring
// tiles share records in one L2), which on the uniform benchmark scene cost +39 % HBM traffic in render_bwd (594
// instead of 428 MB, profiles/r04_pmc_summary_all_tiles_ordered.json) for 2 % of its time; on a skewed scene
// (garden-shaped workload: longest list 7x the average) it is worth 6.5 %.
// (The forward itself keeps the plain XCD-run order: dealt heaviest first by list length it was 10-14 us SLOWER on
// the garden-shaped workload, profiles/r04_tile_order_ab.txt -- the list length says little about a dense tile's
// forward, whose pixels saturate early, and neighbouring tiles no longer run side by side on one XCD's L2.)
inline bool tile_order_pays(long long last_longest, int num_tiles, size_t S) {
  return last_longest > 0 && S > 0 && (last_longest * (long long)num_tiles > 3ll * (long long)S);
}
// The forward splits its long lists only where ONE list sets the launch's duration: the last forward's longest chain
// (the largest stop index of any tile) against `gate` times the work per resident workgroup (the sum over the tiles / 2048).
// A throughput-bound scene gains nothing from the split and pays for its table, its combine pass and the product passes
// (garden-shaped synthetic scene 0.197 -> 0.271 ms, dense4m 0.183 -> 0.26 when split regardless).
inline bool forward_split_pays(long long top_max, long long top_sum, double gate) {
  return top_sum > 0 && (top_max * 2048ll > (long long)(gate * (double)top_sum));
}

// Extra segment blocks of the backward: what the last forward's tiles asked for and half again, at most what `cap`
// instances can hold (gs_render.h: segment_slot).  `seg_entries`: gs_render.h's kSegEntries.
inline size_t bwd_segment_room(size_t cap, size_t asked, size_t seg_entries) {
  return std::min(cap / seg_entries + 2, (asked + asked / 2 + 256 + 7) & ~(size_t)7);
}
// Segment blocks of the forward: asked and a quarter again, at most the sum of ceil(len / seg_entries) over any lists;
// rounded up to eight AFTER the min.
inline size_t fwd_segment_room(size_t cap, int num_tiles, size_t asked, size_t seg_entries) {
  return (std::min(cap / seg_entries + (size_t)num_tiles + 8, asked + asked / 4 + 512) + 7) & ~(size_t)7;
}

// The figures the segment kernels publish -- how uneven the tiles' work is, how many segments the lists asked for --
// decide whether a later forward splits and how much room it reserves, and a split forward sums per-segment
// partials where an unsplit one runs one fma chain: the decision must not follow host / GPU timing.  So each figure is
// written as {ticket << 32 | value}, into the slot of its forward's ticket parity.  Forward `ticket` reads the slot of ticket - 2: the host has seen the record of forward ticket - 1, which was
// published BEHIND everything forward ticket - 2 queued, so that slot is complete, and nobody writes it again before
// this forward's own kernels run.  A word that does not carry ticket - 2 leaves its figure as it was; max and sum go
// together or not at all.
struct Figures {
  long long max = 0, sum = 0;              // largest stop index of any tile, sum over the tiles
  long long asked_bwd = 0, asked_fwd = 0;  // segments / segment blocks the lists asked for
};
inline void take_figures(const unsigned long long w[4], unsigned long long ticket, Figures &f) {
  if (ticket < 3) return;
  const unsigned int want_tag = (unsigned int)((ticket - 2) & 0xFFFFFFFFull);
  if ((unsigned int)(w[0] >> 32) == want_tag && (unsigned int)(w[1] >> 32) == want_tag) {
    f.max = (long long)(int)(unsigned int)w[0];
    f.sum = (long long)(int)(unsigned int)w[1];
  }
  if ((unsigned int)(w[2] >> 32) == want_tag) f.asked_bwd = (long long)(int)(unsigned int)w[2];
  if ((unsigned int)(w[3] >> 32) == want_tag) f.asked_fwd = (long long)(int)(unsigned int)w[3];
}

}  // namespace gs
