// What the canonical-graph builders share (canon.hip, canon_small.hip, clevr_graph.hip): a relation's graph as a bit
// matrix, one 64-bit word = 64 objects of a row; and the rules by which their entries take the rows the host holds.
#pragma once
#include "csg_common.h"

namespace csg {

// ---- a 64x64 bit matrix in one register per lane of a wave64: lane = row

__device__ __forceinline__ int wave_incscan(int v, int lane) {
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int t = __shfl_up(v, o, 64);
    if (lane >= o) v += t;
  }
  return v;
}

// row k of the matrix whose row `lane` is v; k is wave-uniform
__device__ __forceinline__ uint64_t row_of(uint64_t v, int k) {
  const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)v, k);
  const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(v >> 32), k);
  return (uint64_t)hi << 32 | lo;
}

// path() (graphs_utils.py:15-27) over the first n rows: row j takes row i when j -> i, pivots in order
__device__ __forceinline__ uint64_t wave_close(uint64_t row, int n, int lane) {
  for (int i = 0; i < n; ++i) {
    const uint64_t ri = row_of(row, i);
    if (ri == 0) continue;                             // wave-uniform: an empty row adds nothing
    if (lane != i && ((row >> i) & 1ull)) row |= ri;
  }
  return row;
}

// ---- the set bits of a row word, ascending

// the lowest set bit of m, which it loses; m != 0
__device__ __forceinline__ int pop_bit(uint64_t& m) {
  const int k = __ffsll((long long)m) - 1;
  m &= m - 1;
  return k;
}

// one row of the output, if the batch's T rows per sample have room for it: the only place that asks
__device__ __forceinline__ void put_triplet(int64_t* trip, int64_t* tt, int64_t at, int64_t T, int64_t s, int64_t p,
                                            int64_t o, int type) {
  if (at < 0 || at >= T) return;
  trip[at * 3 + 0] = s;
  trip[at * 3 + 1] = p;
  trip[at * 3 + 2] = o;
  tt[at] = type;
}

// (s, p, base + k) for every set bit k of m, from position `at` on; returns the position after them
__device__ __forceinline__ int64_t emit_bits(uint64_t m, int base, int64_t at, int64_t T, int64_t* trip, int64_t* tt, int s,
                                             int p, int type) {
  while (m) put_triplet(trip, tt, at++, T, s, p, base + pop_bit(m), type);
  return at;
}

// ---- a converse draw: searchsorted(cd[0 .. K-2], u, side='right'), the number of those thresholds <= u.  K - 1 = "none":
// the last threshold, cd[K-1] = 1, is never asked.  The bisection equals a scan from the left because cd is non-decreasing:
// the host's cdf is a normalised cumulative sum of non-negative terms (a softmax's).
__device__ __forceinline__ int choice_right(const double* cd, int K, double u) {
  int lo = 0, hi = K - 1;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (cd[mid] <= u) lo = mid + 1; else hi = mid;
  }
  return lo;
}

// ---- entries: what the host holds is checked before anything is enqueued

// `fn`: __padding__ and __in_image__ are two ids of [0, P)
inline int check_meta_ids(const char* fn, int64_t P, int64_t pid_padding, int64_t pid_in_image) {
  CSG_REQUIRE(pid_padding >= 0 && pid_padding < P && pid_in_image >= 0 && pid_in_image < P && pid_padding != pid_in_image,
              CSG_E_BADSHAPE, "%s: __padding__ = %ld and __in_image__ = %ld must be two ids of [0, %ld)", fn, (long)pid_padding,
              (long)pid_in_image, (long)P);
  return CSG_OK;
}

// Row r = t[0 .. 2] = (s, p, o) of sample b, which has n objects, in the host's copy: 1 = a row of the graph, 0 = a
// __padding__ row that is skipped (`skip_padding`; refused otherwise), CSG_E_BADSHAPE = refused, with `fn`'s message;
// `or_padding` is what an entry that can refuse __padding__ appends to its predicate message (" or __padding__"), else "".
inline int check_host_row(const char* fn, bool skip_padding, const char* or_padding, const int64_t* t, int64_t b, int64_t r,
                          int64_t P, int64_t pid_padding, int64_t n) {
  const int64_t s = t[0], p = t[1], o = t[2];
  if (skip_padding && p == pid_padding) return 0;
  CSG_REQUIRE(p >= 0 && p < P && p != pid_padding, CSG_E_BADSHAPE, "%s: sample %ld row %ld: predicate %ld outside [0, %ld)%s",
              fn, (long)b, (long)r, (long)p, (long)P, or_padding);
  CSG_REQUIRE(s >= 0 && s < n && o >= 0 && o < n, CSG_E_BADSHAPE, "%s: sample %ld row %ld: object %ld or %ld outside [0, %ld)",
              fn, (long)b, (long)r, (long)s, (long)o, (long)n);
  return 1;
}

}  // namespace csg
