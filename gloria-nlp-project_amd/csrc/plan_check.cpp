// Stand-alone self-check of the tile planner (glr_plan.cpp), built by `make plan_check` with AddressSanitizer and
// UBSan: seeded random batches planned into heap buffers of EXACTLY glr_plan_size words (an over-run is a sanitizer
// report), the slot and tile-coverage invariants, and the error returns.  Exit status 0 = clean.
#include <stdio.h>

#include <algorithm>
#include <functional>
#include <random>
#include <vector>

#include "../../include/glr.h"

namespace {

int failures = 0;
#define CHECK(cond)                                                            \
  do {                                                                         \
    if (!(cond)) { printf("%s:%d: %s\n", __FILE__, __LINE__, #cond); ++failures; } \
  } while (0)

void check_plan(const std::vector<int32_t>& lens, int capacity, int allow_pairs) {
  const int n = (int)lens.size();
  const int size = glr_plan_size(lens.data(), n, capacity);
  CHECK(size > GLR_PLAN_HEADER);
  if (size <= 0) return;
  std::vector<int32_t> plan(size, -1);                 // capacity == size: the heap block ends with the buffer
  const int used = glr_plan_build(lens.data(), n, capacity, allow_pairs, plan.data(), size);
  CHECK(used > 0 && used <= size && used == plan[GLR_PLAN_N_INTS]);
  if (used <= 0) return;
  const int n_tiles = plan[GLR_PLAN_N_TILES], n_single = plan[GLR_PLAN_N_SINGLE], n_pair = plan[GLR_PLAN_N_PAIR];
  CHECK(plan[GLR_PLAN_N_SENT] == n && plan[GLR_PLAN_CAPACITY] == capacity && n_tiles > 0);
  CHECK(plan[GLR_PLAN_N_LONG_PAIR] >= 0 && plan[GLR_PLAN_N_LONG_PAIR] <= n_pair);
  CHECK(allow_pairs && capacity == GLR_TILE_WORDS ? true : n_pair == 0);
  const int len[8] = {n, n, n_tiles + 1, plan[GLR_PLAN_N_ORDER], n_tiles, n_single, n_pair, 64 * n_pair};
  for (int a = 0; a < 8; ++a) {
    const int off = plan[GLR_PLAN_OFF_CAP_LENS + a];
    CHECK(off >= GLR_PLAN_HEADER && off + len[a] <= used);
    if (off < GLR_PLAN_HEADER || off + len[a] > used) return;
  }
  CHECK(plan[GLR_PLAN_OFF_PAIR_DESC] % 64 == 0);
  const int32_t* slot0 = plan.data() + plan[GLR_PLAN_OFF_SENT_SLOT0];
  const int32_t* nsub = plan.data() + plan[GLR_PLAN_OFF_TILE_NSUB];
  const int32_t* single = plan.data() + plan[GLR_PLAN_OFF_SINGLE_TILE];
  const int32_t* pair = plan.data() + plan[GLR_PLAN_OFF_PAIR_TILE];
  // every word has a slot of its own, inside the populated part of a tile
  std::vector<char> slot_used((size_t)n_tiles * GLR_TILE_WORDS, 0);
  for (int i = 0; i < n; ++i)
    for (int w = 0; w < lens[i]; ++w) {
      const int slot = slot0[i] + (w / capacity) * GLR_TILE_WORDS + w % capacity;
      CHECK(slot >= 0 && slot < n_tiles * GLR_TILE_WORDS);
      if (slot < 0 || slot >= n_tiles * GLR_TILE_WORDS) return;
      CHECK(!slot_used[slot] && slot % GLR_TILE_WORDS < capacity);
      slot_used[slot] = 1;
    }
  // the work items cover every tile exactly once
  std::vector<int> covered(n_tiles, 0);
  auto cover = [&](int t0, int k) {
    CHECK(t0 >= 0 && t0 + k <= n_tiles);
    for (int t = t0; t < t0 + k && t >= 0 && t < n_tiles; ++t) ++covered[t];
  };
  for (int k = 0; k < n_pair; ++k) {
    cover(pair[k], 2);
    CHECK((nsub[pair[k]] == 2) == (k < plan[GLR_PLAN_N_LONG_PAIR]));
  }
  for (int k = 0; k < n_single; ++k) cover(single[k], std::max(nsub[single[k]], 1));
  CHECK(std::count(covered.begin(), covered.end(), 1) == n_tiles);
  // one word short: refused
  std::vector<int32_t> tight(used - 1);
  CHECK(glr_plan_build(lens.data(), n, capacity, allow_pairs, tight.data(), used - 1) == GLR_EINVAL);
}

}  // namespace

int main() {
  std::mt19937 rng(123);
  auto draw = [&](int lo, int hi) { return lo + (int)(rng() % (unsigned)(hi - lo + 1)); };
  int batches = 0;
  for (int trial = 0; trial < 40; ++trial) {
    const int maxima[5] = {8, 40, 97, 257, 512};
    std::vector<int32_t> lens(draw(1, 300));
    for (auto& v : lens) v = draw(1, maxima[trial % 5]);
    for (int capacity : {64, 32})
      for (int allow_pairs : {0, 1}) { check_plan(lens, capacity, allow_pairs); ++batches; }
  }
  for (unsigned seed : {1234u, 1u, 2u}) {            // the bench's shape: 256 captions of 5..40 words, longest first
    rng.seed(seed);
    std::vector<int32_t> lens(256);
    for (auto& v : lens) v = draw(4, 39) + 1;
    std::sort(lens.begin(), lens.end(), std::greater<int32_t>());
    for (int capacity : {64, 32})
      for (int allow_pairs : {0, 1}) { check_plan(lens, capacity, allow_pairs); ++batches; }
  }
  // error returns
  std::vector<int32_t> out(4096);
  const int32_t zero_len[3] = {3, 0, 2}, long_len[1] = {GLR_MAX_WORDS + 1}, ok[2] = {5, 70};
  CHECK(glr_plan_size(zero_len, 3, 64) == GLR_EINVAL && glr_plan_build(zero_len, 3, 64, 1, out.data(), 4096) == GLR_EINVAL);
  CHECK(glr_plan_size(long_len, 1, 64) == GLR_EINVAL && glr_plan_build(long_len, 1, 64, 1, out.data(), 4096) == GLR_EINVAL);
  CHECK(glr_plan_size(ok, 0, 64) == GLR_EINVAL && glr_plan_build(ok, 0, 64, 1, out.data(), 4096) == GLR_EINVAL);
  CHECK(glr_plan_size(nullptr, 2, 64) == GLR_EINVAL && glr_plan_build(nullptr, 2, 64, 1, out.data(), 4096) == GLR_EINVAL);
  CHECK(glr_plan_build(ok, 2, 64, 1, nullptr, 4096) == GLR_EINVAL);
  CHECK(glr_plan_size(ok, 2, 48) == GLR_EINVAL && glr_plan_build(ok, 2, 48, 1, out.data(), 4096) == GLR_EINVAL);
  CHECK(glr_plan_build(ok, 2, 64, 1, out.data(), 0) == GLR_EINVAL);
  printf("plan_check: %d plans, %d failures\n", batches, failures);
  return failures ? 1 : 0;
}
