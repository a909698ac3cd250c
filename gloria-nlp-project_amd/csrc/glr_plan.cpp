// Host-side tile planning: plain C++ (no HIP), one call.  glr_plan_build replaces the per-sentence slice
// words_emb[i, :, :cap_lens[i]] of the reference loop (gloria/loss/gloria_loss.py:116-123) by a packed slot table
// and lists the work items of the K1 kernels; everything lands in ONE int32 buffer (layout: include/glr.h) that the
// caller uploads once and hands to glr_pack_words / glr_local_attn_fwd / glr_local_attn_bwd.
#include <limits.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "../../include/glr.h"

namespace {

// tiles needed when every sentence is packed alone: >= number of tiles, == number of `order` entries
int plan_bound(const int32_t* cap_lens, int n_sent, int capacity) {
  if (!cap_lens || n_sent <= 0 || (capacity != 32 && capacity != GLR_TILE_WORDS)) return GLR_EINVAL;
  long long total = 0;
  for (int i = 0; i < n_sent; ++i) {
    if (cap_lens[i] < 1 || cap_lens[i] > GLR_MAX_WORDS) return GLR_EINVAL;
    total += (cap_lens[i] + capacity - 1) / capacity;
  }
  return total > INT_MAX / 64 ? GLR_EINVAL : (int)total;
}

// Sentences -> tiles.  A sentence of at most `capacity` words lies inside one tile (first fit, in the given order); a
// longer one owns ceil(n / capacity) consecutive tiles.  max_pair_seg 0: plain first fit; > 1: tiles will be paired, a
// pair holding at most that many sentences.  Returns the number of tiles.
int plan_tiles(const int32_t* cap_lens, int n_sent, int capacity, int max_pair_seg, int32_t* sent_slot0,
               int32_t* tile_first, int32_t* order, int32_t* tile_nsub) {
  std::vector<int> fill;                       // used slots per tile (capacity = closed)
  std::vector<std::vector<int>> members;
  std::vector<int> nsub;
  // first fit in caption order, at most `max_sent` sentences per ordinary tile
  auto pack = [&](int max_sent) {
    fill.clear(); members.clear(); nsub.clear();
    for (int i = 0; i < n_sent; ++i) {
      const int n = cap_lens[i];
      if (n > capacity) {                      // multi-tile sentence: its own run of consecutive tiles
        const int k = (n + capacity - 1) / capacity;
        for (int s = 0; s < k; ++s) {
          fill.push_back(capacity);
          members.emplace_back(1, i);
          nsub.push_back(s == 0 ? k : -1);
        }
        continue;
      }
      size_t t = 0;
      while (t < fill.size() && (fill[t] + n > capacity || (int)members[t].size() >= max_sent)) ++t;
      if (t == fill.size()) { fill.push_back(0); members.emplace_back(); nsub.push_back(0); }
      fill[t] += n;
      members[t].push_back(i);
    }
  };
  // work items the pair kernels would need for the current packing: ordinary tiles sorted by sentence count and
  // paired fewest-with-most (the order built below), a pair holding at most max_pair_seg sentences
  auto items = [&]() {
    std::vector<int> cnt;
    int n_items = 0;
    for (size_t t = 0; t < members.size(); ++t) {
      if (nsub[t] == 0) cnt.push_back((int)members[t].size());
      else if (nsub[t] > 0) ++n_items;
    }
    std::sort(cnt.begin(), cnt.end());
    std::vector<int> seq;
    for (size_t lo = 0, hi = cnt.size(); lo < hi;) {
      seq.push_back(cnt[lo++]);
      if (lo < hi) seq.push_back(cnt[--hi]);
    }
    for (size_t t = 0; t < seq.size();) {
      if (t + 1 < seq.size() && seq[t] + seq[t + 1] <= max_pair_seg) t += 2; else t += 1;
      ++n_items;
    }
    return n_items;
  };
  // Plain first fit leaves the many short sentences of a length-sorted batch in the last tiles, which then hold more
  // sentences than a pair may (max_pair_seg) and run as single tiles - a workgroup each, like a whole pair.  With
  // pairing in view, a cap on the sentences per tile is chosen that minimises the number of work items (ties: fewer
  // tiles): a tile more usually costs less than the pairs it unlocks.
  int best_cap = n_sent;
  if (max_pair_seg > 1) {
    long best_cost = -1;
    for (int cap = max_pair_seg; cap >= max_pair_seg / 2; --cap) {
      pack(cap == max_pair_seg ? n_sent : cap);
      const long cost = (long)items() * 4096 + (long)members.size();
      if (best_cost < 0 || cost < best_cost) { best_cost = cost; best_cap = cap == max_pair_seg ? n_sent : cap; }
    }
  }
  pack(best_cap);
  // Tile ORDER is free (a tile is just 64 consecutive slots): multi-tile sentences first (their runs stay
  // together), then the ordinary tiles, contiguous - the pair kernels take two CONSECUTIVE ordinary tiles - and
  // balanced: fewest sentences next to most, second fewest next to second most, ...
  {
    std::vector<size_t> by_cnt, seq;
    for (size_t t = 0; t < members.size(); ++t) if (nsub[t] != 0) seq.push_back(t);
    for (size_t t = 0; t < members.size(); ++t) if (nsub[t] == 0) by_cnt.push_back(t);
    std::stable_sort(by_cnt.begin(), by_cnt.end(), [&](size_t a, size_t b) { return members[a].size() < members[b].size(); });
    for (size_t lo = 0, hi = by_cnt.size(); lo < hi;) {
      seq.push_back(by_cnt[lo++]);
      if (lo < hi) seq.push_back(by_cnt[--hi]);
    }
    std::vector<std::vector<int>> m2(members.size());
    std::vector<int> f2(fill.size()), n2(nsub.size());
    for (size_t i = 0; i < seq.size(); ++i) { m2[i] = members[seq[i]]; f2[i] = fill[seq[i]]; n2[i] = nsub[seq[i]]; }
    members.swap(m2);
    fill.swap(f2);
    nsub.swap(n2);
    for (size_t t = 0; t < members.size(); ++t) {
      if (nsub[t] != 0) continue;
      int pos = 0;
      for (int s : members[t]) { sent_slot0[s] = (int)t * GLR_TILE_WORDS + pos; pos += cap_lens[s]; }
    }
  }
  for (size_t t = 0; t < members.size(); ++t)
    if (nsub[t] > 0) sent_slot0[members[t][0]] = (int)t * GLR_TILE_WORDS;
  int k = 0;
  for (size_t t = 0; t < members.size(); ++t) {
    tile_first[t] = k;
    tile_nsub[t] = nsub[t];
    for (int s : members[t]) order[k++] = s;
  }
  tile_first[members.size()] = k;
  return (int)members.size();
}

// Work items of the K1 kernels.  With allow_pairs, two consecutive ordinary tiles that hold at most
// GLR_MAX_PAIR_SEG sentences IN TOTAL become one work item, and so do the two tiles of ONE 65..128-word sentence.
int plan_items(const int32_t* tile_nsub, const int32_t* tile_first, int n_tiles, bool allow_pairs, int32_t* single_tile,
               int32_t* pair_tile, int* n_single, int* n_pair) {
  int ns = 0, np = 0;
  auto pairable = [&](int t) { return t < n_tiles && tile_nsub[t] == 0; };
  for (int t = 0; t < n_tiles;) {
    if (tile_nsub[t] < 0) return GLR_EINVAL;         // a continuation tile cannot start an item
    if (tile_nsub[t] == 2 && allow_pairs) {          // a 65..128-word sentence owns exactly one pair of tiles
      pair_tile[np++] = t;
      t += 2;
    } else if (tile_nsub[t] > 1) {                   // longer sentence: one item, handled in sweeps
      single_tile[ns++] = t;
      t += tile_nsub[t];
    } else if (allow_pairs && pairable(t) && pairable(t + 1) && tile_first[t + 2] - tile_first[t] <= GLR_MAX_PAIR_SEG) {
      pair_tile[np++] = t;
      t += 2;
    } else {
      single_tile[ns++] = t;
      t += 1;
    }
  }
  *n_single = ns; *n_pair = np;
  return GLR_OK;
}

// Row flags of the pair kernels, for tile t (head = first tile of its sentence when the sentence owns whole tiles).
// There a wave holds ALL 64 word slots of a tile for its region columns: lane half h (lane >> 5) owns the slots w with
// ((w >> 2) & 1) == h, 32 rows in word order, row index k(w) = 16 (w >> 5) + 4 ((w & 31) >> 3) + (w & 3) (the
// accumulator register, second 32-word block at k >= 16).  The words of a sentence are a run of rows in each half; the
// kernel walks the rows once per pass and only acts where a run starts or ends, which is the same for all lanes of a
// half: per tile and half one bit per row.
//   f[0..1]  START bits of half 0 / 1: first row of a sentence's run
//   f[2..3]  LAST  bits: last row of a run
//   f[4..5]  OWNER bits (subset of START): the run that holds the sentence's first word (that lane half stores the
//            sentence's log-sum-exp row for the backward pass)
//   f[6..7]  reserved (0)
int plan_rowflags(const int32_t* cap_lens, const int32_t* sent_slot0, const int32_t* tile_first, const int32_t* order,
                  const int32_t* tile_nsub, int t, int head, int32_t* f) {
  auto row_of = [](int w) { return 16 * (w >> 5) + 4 * ((w & 31) >> 3) + (w & 3); };
  uint32_t u[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  for (int k = tile_first[t]; k < tile_first[t + 1]; ++k) {
    const int sent = order[k];
    int a, e;
    bool owner = true;
    if (tile_nsub[t] == 0) {
      a = sent_slot0[sent] - t * GLR_TILE_WORDS;
      e = a + cap_lens[sent];
    } else {                                                // tile (t - head) of a sentence that owns whole tiles
      const int sub = t - head;
      a = 0;
      e = std::min(cap_lens[sent] - sub * GLR_TILE_WORDS, GLR_TILE_WORDS);
      owner = sub == 0;
    }
    if (a < 0 || e > GLR_TILE_WORDS || e <= a) return GLR_EINVAL;
    int first[2] = {-1, -1}, last[2] = {-1, -1};
    for (int w = a; w < e; ++w) {
      const int hh = (w >> 2) & 1;
      if (first[hh] < 0) first[hh] = w;
      last[hh] = w;
    }
    for (int hh = 0; hh < 2; ++hh) {
      if (first[hh] < 0) continue;
      u[hh] |= 1u << row_of(first[hh]);
      u[2 + hh] |= 1u << row_of(last[hh]);
      if (owner && first[hh] == a) u[4 + hh] |= 1u << row_of(first[hh]);
    }
  }
  for (int q = 0; q < 8; ++q) f[q] = (int32_t)u[q];
  return GLR_OK;
}

// Pair descriptors: everything a workgroup needs to know about its pair of tiles in ONE coalesced 256-byte read
// (instead of dependent global round trips through tile_first / order / sent_slot0 / cap_lens); layout: include/glr.h
int plan_pair_desc(const int32_t* cap_lens, const int32_t* sent_slot0, const int32_t* tile_first, const int32_t* order,
                   const int32_t* tile_nsub, int n_tiles, const int32_t* pair_tile, int n_pair, int32_t* desc) {
  memset(desc, 0, sizeof(int32_t) * 64 * (size_t)n_pair);
  for (int k = 0; k < n_pair; ++k) {
    const int t0 = pair_tile[k];
    if (t0 < 0 || t0 + 1 >= n_tiles) return GLR_EINVAL;
    int32_t* d = desc + 64 * (size_t)k;
    const bool lp = tile_nsub[t0] == 2;
    const int ns = lp ? 1 : tile_first[t0 + 2] - tile_first[t0];
    if (ns < 1 || ns > GLR_MAX_PAIR_SEG) return GLR_EINVAL;
    d[0] = ns;
    d[1] = lp ? 1 : 0;
    for (int s = 0; s < ns; ++s) {
      const int sent = order[tile_first[t0] + s];
      d[8 + s] = sent;
      d[16 + s] = sent_slot0[sent] - t0 * GLR_TILE_WORDS;
      d[24 + s] = cap_lens[sent];
    }
    for (int half = 0; half < 2; ++half) {
      const int rc = plan_rowflags(cap_lens, sent_slot0, tile_first, order, tile_nsub, t0 + half, t0, d + 32 + 8 * half);
      if (rc != GLR_OK) return rc;
    }
  }
  return GLR_OK;
}

}  // namespace

extern "C" int glr_plan_size(const int32_t* cap_lens, int n_sent, int capacity) {
  const int bound = plan_bound(cap_lens, n_sent, capacity);
  if (bound < 0) return bound;
  // header | cap_lens, sent_slot0 | tile_first | order | tile_nsub, single_tile, pair_tile | alignment | pair_desc
  const long long n = GLR_PLAN_HEADER + 2LL * n_sent + (bound + 1) + bound + 3LL * bound + 63 + 64LL * (bound / 2);
  return n > INT_MAX ? GLR_EINVAL : (int)n;
}

extern "C" int glr_plan_build(const int32_t* cap_lens, int n_sent, int capacity, int allow_pairs, int32_t* plan,
                              int plan_ints) {
  const int bound = plan_bound(cap_lens, n_sent, capacity);
  if (bound < 0) return bound;
  if (!plan) return GLR_EINVAL;
  const bool pairing = allow_pairs && capacity == GLR_TILE_WORDS;     // the pair kernels run full-width (bf16) tiles only
  std::vector<int32_t> sent_slot0(n_sent), tile_first(bound + 1), order(bound), tile_nsub(bound), single_tile(bound),
      pair_tile(bound);
  const int n_tiles = plan_tiles(cap_lens, n_sent, capacity, pairing ? GLR_MAX_PAIR_SEG : 0, sent_slot0.data(),
                                 tile_first.data(), order.data(), tile_nsub.data());
  int n_single = 0, n_pair = 0;
  int rc = plan_items(tile_nsub.data(), tile_first.data(), n_tiles, pairing, single_tile.data(), pair_tile.data(),
                      &n_single, &n_pair);
  if (rc != GLR_OK) return rc;
  // the pairs that are the two tiles of ONE 65..128-word sentence lead the pair list (multi-tile sentences are planned
  // first): the K1 entry points route that prefix and the rest to different kernels
  int n_long_pair = 0;
  while (n_long_pair < n_pair && tile_nsub[pair_tile[n_long_pair]] == 2) ++n_long_pair;
  for (int k = n_long_pair; k < n_pair; ++k)
    if (tile_nsub[pair_tile[k]] == 2) return GLR_EINVAL;
  const int n_order = tile_first[n_tiles];

  const int32_t* src[8] = {cap_lens, sent_slot0.data(), tile_first.data(), order.data(), tile_nsub.data(),
                           single_tile.data(), pair_tile.data(), nullptr};
  const int len[8] = {n_sent, n_sent, n_tiles + 1, n_order, n_tiles, n_single, n_pair, 64 * n_pair};
  int off[8], o = GLR_PLAN_HEADER;
  for (int a = 0; a < 8; ++a) {
    if (a == 7) o = (o + 63) / 64 * 64;          // descriptors on a 256-byte boundary (16-byte LDS-DMA pieces)
    off[a] = o;
    o += len[a];
  }
  if (plan_ints < o) return GLR_EINVAL;
  memset(plan, 0, sizeof(int32_t) * (size_t)o);
  plan[GLR_PLAN_N_SENT] = n_sent; plan[GLR_PLAN_N_TILES] = n_tiles; plan[GLR_PLAN_CAPACITY] = capacity;
  plan[GLR_PLAN_N_ORDER] = n_order; plan[GLR_PLAN_N_SINGLE] = n_single; plan[GLR_PLAN_N_PAIR] = n_pair;
  plan[GLR_PLAN_N_LONG_PAIR] = n_long_pair; plan[GLR_PLAN_N_INTS] = o;
  for (int a = 0; a < 8; ++a) {
    plan[GLR_PLAN_OFF_CAP_LENS + a] = off[a];
    if (src[a] && len[a] > 0) memcpy(plan + off[a], src[a], sizeof(int32_t) * (size_t)len[a]);
  }
  if (n_pair > 0)
    rc = plan_pair_desc(cap_lens, sent_slot0.data(), tile_first.data(), order.data(), tile_nsub.data(), n_tiles,
                        pair_tile.data(), n_pair, plan + off[7]);
  return rc == GLR_OK ? o : rc;
}
