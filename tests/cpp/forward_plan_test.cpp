// The forward's host decisions (3dgs_amd/csrc/gs_forward_plan.h) on hand-worked cases.  Host only: built with g++ and
// the address / undefined-behaviour sanitizers by tests/test_forward_plan_cpu.py and run as a stand-alone program.
#include "gs_forward_plan.h"

#include <cstdio>

static int failures = 0;
#define CHECK(expr)                                                   \
  do {                                                                \
    if (!(expr)) {                                                    \
      std::printf("FAILED line %d: %s\n", __LINE__, #expr);           \
      ++failures;                                                     \
    }                                                                 \
  } while (0)

static unsigned long long tagged(unsigned long long tag, unsigned int value) { return (tag << 32) | value; }

int main() {
  using namespace gs;
  constexpr size_t kSeg = 496;  // entries per segment the room cases were worked for

  CHECK(compact_walk(1000, 799, 1000));
  CHECK(!compact_walk(1000, 800, 1000));
  CHECK(!compact_walk(1000, 0, 1000));
  CHECK(!compact_walk(999, 10, 1000));
  CHECK(compact_walk(64 << 20, 1, 64 << 20));  // (5 * 2^26 and 4 * 2^26 do not fit an int)

  CHECK(sort_class(-1, true) == 0);
  CHECK(sort_class(1024, true) == 0);
  CHECK(sort_class(1025, true) == 1);
  CHECK(sort_class(2048, true) == 1);
  CHECK(sort_class(2049, true) == 2);
  CHECK(sort_class(4096, true) == 2);
  CHECK(sort_class(4097, true) == 3);
  CHECK(sort_class(8192, true) == 3);
  CHECK(sort_class(8193, true) == 4);
  CHECK(sort_class(1024, false) == 1);

  CHECK(speculative_longest(-1) == -1);
  CHECK(speculative_longest(0) == 64);
  CHECK(speculative_longest(1000) == 1564);

  CHECK(!tail_needs_redo(100, 100, -1, 9000, true));
  CHECK(tail_needs_redo(101, 100, -1, 10, true));
  CHECK(!tail_needs_redo(10, 100, 1564, 1500, true));
  CHECK(tail_needs_redo(10, 100, 1564, 2049, true));
  CHECK(!tail_needs_redo(10, 100, 64, 1000, true));
  CHECK(!tail_needs_redo(10, 100, 64, 1000, false));

  CHECK(!tile_order_pays(-1, 8160, 1000));
  CHECK(!tile_order_pays(300, 100, 10000));
  CHECK(tile_order_pays(301, 100, 10000));
  CHECK(!tile_order_pays(5, 100, 0));
  CHECK(tile_order_pays(2147483647ll, 16384, 1));

  CHECK(!forward_split_pays(3000, 2048000, 3.0));
  CHECK(forward_split_pays(3001, 2048000, 3.0));
  CHECK(!forward_split_pays(1, 0, 3.0));
  CHECK(forward_split_pays(1, 5, 0.0));
  CHECK(!forward_split_pays(0, 5, 0.0));

  CHECK(bwd_segment_room(1000000, 0, kSeg) == 256);
  CHECK(bwd_segment_room(1000000, 1001, kSeg) == 1760);
  CHECK(bwd_segment_room(1000, 100, kSeg) == 4);

  CHECK(fwd_segment_room(1000000, 8160, 0, kSeg) == 512);
  CHECK(fwd_segment_room(1000000, 8160, 1001, kSeg) == 1768);
  CHECK(fwd_segment_room(1000, 4, 1000, kSeg) == 16);  // min(14, 1762) = 14, THEN rounded up to eight

  {  // ticket 2: nothing is taken, whatever the tags say
    const unsigned long long w[4] = {tagged(0, 11), tagged(0, 12), tagged(0, 13), tagged(0, 14)};
    Figures f = {1, 2, 3, 4};
    take_figures(w, 2, f);
    CHECK(f.max == 1 && f.sum == 2 && f.asked_bwd == 3 && f.asked_fwd == 4);
  }
  {  // ticket 5, all four words from forward 3
    const unsigned long long w[4] = {tagged(3, 11), tagged(3, 12), tagged(3, 13), tagged(3, 14)};
    Figures f = {1, 2, 3, 4};
    take_figures(w, 5, f);
    CHECK(f.max == 11 && f.sum == 12 && f.asked_bwd == 13 && f.asked_fwd == 14);
  }
  {  // the sum is from forward 1: max AND sum stay, the two "asked" figures are taken
    const unsigned long long w[4] = {tagged(3, 11), tagged(1, 12), tagged(3, 13), tagged(3, 14)};
    Figures f = {1, 2, 3, 4};
    take_figures(w, 5, f);
    CHECK(f.max == 1 && f.sum == 2 && f.asked_bwd == 13 && f.asked_fwd == 14);
  }
  {  // only the backward's figure is from forward 3
    const unsigned long long w[4] = {tagged(1, 11), tagged(1, 12), tagged(3, 13), tagged(1, 14)};
    Figures f = {1, 2, 3, 4};
    take_figures(w, 5, f);
    CHECK(f.max == 1 && f.sum == 2 && f.asked_bwd == 13 && f.asked_fwd == 4);
  }
  {  // ticket 2^32 + 1: the wanted tag is the low half of 2^32 - 1
    const unsigned long long w[4] = {tagged(0xFFFFFFFFull, 11), tagged(0xFFFFFFFFull, 12), tagged(0, 13), tagged(0xFFFFFFFEull, 14)};
    Figures f = {1, 2, 3, 4};
    take_figures(w, (1ull << 32) + 1, f);
    CHECK(f.max == 11 && f.sum == 12 && f.asked_bwd == 3 && f.asked_fwd == 4);
  }
  {  // a value with its top bit set keeps its sign (the kernels publish ints)
    const unsigned long long w[4] = {tagged(3, 0xFFFFFFFFu), tagged(3, 12), tagged(3, 13), tagged(3, 14)};
    Figures f = {1, 2, 3, 4};
    take_figures(w, 5, f);
    CHECK(f.max == -1 && f.sum == 12);
  }

  {
    const unsigned long long ticket = (7ull << 32) | 0x80000009ull;  // (only the low half travels)
    const unsigned long long pairs = 0x123456789ull;
    unsigned long long w[kRecordWords] = {record_word(4321u, ticket), record_word(98765u, ticket),
                                          record_word((unsigned int)(pairs & 0xFFFFFFFFull), ticket),
                                          record_word((unsigned int)(pairs >> 32), ticket), record_word(777u, ticket)};
    CHECK(record_arrived(w, ticket));
    for (int k = 0; k < kRecordWords; ++k) {  // any one word still carrying the previous forward's ticket
      const unsigned long long keep = w[k];
      w[k] = record_word((unsigned int)(keep >> 32), ticket - 1);
      CHECK(!record_arrived(w, ticket));
      w[k] = keep;
    }
    const ForwardRecord r = decode_record(w);
    CHECK(r.M == 4321 && r.S == 98765u && r.longest == 777);
    CHECK(r.pairs == pairs);
  }

  if (failures) {
    std::printf("%d checks failed\n", failures);
    return 1;
  }
  std::printf("all checks passed\n");
  return 0;
}
