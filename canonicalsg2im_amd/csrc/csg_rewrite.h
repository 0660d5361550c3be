// Graph rewriting (rewrite.hip): the counter-based hash and the two row rules, written ONCE for the host and the device.
// Integers only: what the host computes with these functions and what a kernel computes are the same bits, and
// tests/rewrite_cases.py restates them in numpy uint64.
//
//   fin(z)   = the splitmix64 finaliser:  z ^= z >> 30; z *= 0xbf58476d1ce4e5b9; z ^= z >> 27; z *= 0x94d049bb133111eb;
//              z ^= z >> 31
//   step(h, w) = fin((h ^ w) + 0x9e3779b97f4a7c15)
//   h(seed, image, a, b, slot) = step(step(step(step(0, seed), image), a << 32 | b), slot)          -- four words
//   a row is SELECTED when (h >> 32) < threshold, threshold = floor(share * 2^32 + 0.5) in [0, 2^32]: share 0 never
//   fires, share 1 always does.  One more round, g = step(h, 1), gives the coin (g >> 63) and the replacement index
//   ((g >> 32) * 5) >> 32 in 0..4.
// Slots are those of augmented_relations: below 0, above 1, left of 2, right of 3, inside 4, surrounding 5; the converse
// of slot k is k ^ 1; the FORWARD predicates are above, left of, inside (slots 1, 2, 4).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define CSG_RW_HD __host__ __device__ __forceinline__
#else
#define CSG_RW_HD static inline
#endif

#include "../../include/csg_hip.h"             // CSG_REWRITE_ONE_SIDED / _NOISE, CSG_REWRITE_FORWARD / _BACKWARD / _RANDOM

namespace csg {

CSG_RW_HD uint64_t rw_fin(uint64_t z) {
  z ^= z >> 30;
  z *= 0xbf58476d1ce4e5b9ull;
  z ^= z >> 27;
  z *= 0x94d049bb133111ebull;
  z ^= z >> 31;
  return z;
}

CSG_RW_HD uint64_t rw_step(uint64_t h, uint64_t w) { return rw_fin((h ^ w) + 0x9e3779b97f4a7c15ull); }

// s and o are object rows of a batch: below 2^31 (the entry's limit on O)
CSG_RW_HD uint64_t rw_hash(uint64_t seed, uint64_t image, int64_t a, int64_t b, int slot) {
  uint64_t h = rw_step(0ull, seed);
  h = rw_step(h, image);
  h = rw_step(h, ((uint64_t)a << 32) | (uint64_t)b);
  return rw_step(h, (uint64_t)slot);
}

CSG_RW_HD bool rw_selected(uint64_t h, uint64_t threshold) { return (h >> 32) < threshold; }
CSG_RW_HD bool rw_forward_slot(int slot) { return slot == 1 || slot == 2 || slot == 4; }

// share in [0, 1] -> [0, 2^32]; the caller has refused everything else (a NaN included)
static inline uint64_t rw_threshold(double share) { return (uint64_t)(share * 4294967296.0 + 0.5); }

// one_sided: the row (s, slot, o), rewritten in place.  The pair key is the row's forward form.
CSG_RW_HD void rw_one_sided(uint64_t seed, uint64_t image, uint64_t threshold, int direction, int64_t& s, int& slot, int64_t& o) {
  const bool fwd = rw_forward_slot(slot);
  const int64_t a = fwd ? s : o, b = fwd ? o : s;
  const int kf = fwd ? slot : (slot ^ 1);
  const uint64_t h = rw_hash(seed, image, a, b, kf);
  if (!rw_selected(h, threshold)) return;
  bool want_fwd = direction == CSG_REWRITE_FORWARD;
  if (direction == CSG_REWRITE_RANDOM) want_fwd = (rw_step(h, 1ull) >> 63) == 0ull;
  s = want_fwd ? a : b;
  o = want_fwd ? b : a;
  slot = want_fwd ? kf : (kf ^ 1);
}

// noise: the predicate replaced by one of the other five, uniformly, by ascending slot.  The key is the row as given.
CSG_RW_HD void rw_noise(uint64_t seed, uint64_t image, uint64_t threshold, int64_t s, int& slot, int64_t o) {
  const uint64_t h = rw_hash(seed, image, s, o, slot);
  if (!rw_selected(h, threshold)) return;
  const int r = (int)(((rw_step(h, 1ull) >> 32) * 5ull) >> 32);
  slot = r < slot ? r : r + 1;
}

}  // namespace csg
