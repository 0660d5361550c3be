// The graph of the unpacked CLEVR dataset, one block per sample (csg_clevr_graph_*).  Reference: extract_triplets,
// sg2im/data/clevr_dialog.py:289-307, and reduce_transitive_edges, scripts/graphs_utils.py:15-44,74-82.
//
// The host lists a sample's relation rows [o2, pred, o1] as extract_triplets generates them.  Per predicate, in the order
// in which the predicates first appear among the rows:
//   fewer than 3 listed rows (duplicates counted): the rows as listed (graphs_utils.py:75-76);
//   otherwise: M = the rows as a bit matrix, C = path(M), H = hsu(C) in the reference's in-place order, and the rows of
//   H (keep = 0) or H | M (keep = 1), row-major.
// Then [i, __in_image__, n] for the n objects and [0, __padding__, 0] up to T.  No np.unique, no converse draws, no extras:
// neither csg_canon_small_* nor csg_canon_general_* emit in this order, and their closure has no reduction.
//
// hsu() on a matrix that is not a strict order.  The reference loops j, then i ascending, then clears m[i][k] for every k
// of row j — row j as it is AT THAT MOMENT.  With old = row j before step j and self = bit j of old:
//   i < j with bit j: row i &= ~old;
//   i = j with self:  row j clears itself bit by bit: 0;
//   i > j with bit j: row j is 0 by now when self, so row i &= ~old only if not self.
// For strict orders (CLEVR's own relations) self is never set and this is the textbook reduction.
//
// A sample has at most 64 rows with its __image__ row, so a predicate's matrix is one 64-bit word per lane of a wave, as
// in canon_small.hip: a wave owns a predicate, row k is fetched with two v_readlane (k is the loop counter), and the
// counts are wave scans.  The rows are scattered with LDS atomics (OR, min, max, add on integers: the bytes do not depend
// on the order in which waves run).  Both launches run this same computation from the rows — a few thousand integer
// operations — and differ in what they store: the count launch the sample's number of triplets, the emit launch, after the
// host has read the counts for T, the triplets.  Nothing is kept between them but the rows themselves.
#include "csg_common.h"

using namespace csg;

namespace {

constexpr int GMAXN = 64;        // rows per sample, the __image__ row included: objects are lanes 0 .. 62
constexpr int GMAXP = 16;        // predicates of a vocabulary (CLEVR's has 6)
constexpr int GNW = 4;           // waves per block: one per relation of CLEVR; a wave takes predicates wave, wave + GNW, ...
constexpr int GNT = GNW * 64;

struct GraphParams {
  int P, O, R;
  int pid_padding, pid_in_image;
  int keep;
};

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

__device__ __forceinline__ void put(int64_t* trip, int64_t* tt, int64_t at, int64_t T, int64_t s, int64_t p, int64_t o) {
  if (at < 0 || at >= T) return;
  trip[at * 3 + 0] = s;
  trip[at * 3 + 1] = p;
  trip[at * 3 + 2] = o;
  tt[at] = 0;                                          // ORIGINAL_EDGE; 0 on padding too
}

template <bool EMIT>
__global__ __launch_bounds__(GNT) void k_clevr_graph(GraphParams G, const int64_t* __restrict__ n_rows,
                                                     const int64_t* __restrict__ rel, int64_t* __restrict__ counts,
                                                     int64_t T, int64_t* __restrict__ triplets,
                                                     int64_t* __restrict__ ttype) {
  __shared__ unsigned long long M[GMAXP][GMAXN];       // the listed rows, then the result, of every predicate
  __shared__ int first[GMAXP], last[GMAXP], listed[GMAXP], out_n[GMAXP], base[GMAXP];
  __shared__ int bad, total;
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int P = G.P;
  int n = (int)n_rows[b] - 1;                          // objects: the sample's rows without its __image__ row
  n = n < 0 ? 0 : (n > GMAXN - 1 ? GMAXN - 1 : n);
  if (n > G.O - 1) n = G.O - 1;

  for (int i = tid; i < GMAXP * GMAXN; i += GNT) (&M[0][0])[i] = 0;
  if (tid < GMAXP) {
    first[tid] = 0x7fffffff;
    last[tid] = -1;
    listed[tid] = out_n[tid] = base[tid] = 0;
  }
  if (tid == 0) bad = 0;
  __syncthreads();

  // ---- scatter: M[p][s] bit o; the first and the last listed row of p and how many there are, duplicates counted
  const int64_t* rows = rel + (int64_t)b * G.R * 3;
  for (int r = tid; r < G.R; r += GNT) {
    const int64_t s = rows[r * 3 + 0], p = rows[r * 3 + 1], o = rows[r * 3 + 2];
    if (p == G.pid_padding) continue;
    // the host refused such a row from its copy; a device buffer that disagrees is not indexed with
    if (p < 0 || p >= P || s < 0 || s >= n || o < 0 || o >= n) {
      bad = 1;
      continue;
    }
    atomicOr(&M[p][s], 1ull << o);
    atomicMin(&first[p], r);
    atomicMax(&last[p], r);
    atomicAdd(&listed[p], 1);
  }
  __syncthreads();

  // ---- reduce: a wave per predicate, a lane per row
  for (int p = wave; p < P; p += GNW) {
    const int c = listed[p];
    if (c < 3) {                                       // graphs_utils.py:75-76: as listed
      if (lane == 0) out_n[p] = c;
      continue;
    }
    const uint64_t m = M[p][lane];
    uint64_t row = m;
    for (int i = 0; i < n; ++i) {                      // path(): row j takes row i when j -> i, pivots in order
      const uint64_t ri = row_of(row, i);
      if (ri == 0) continue;                           // wave-uniform: an empty row adds nothing
      if (lane != i && ((row >> i) & 1ull)) row |= ri;
    }
    for (int j = 0; j < n; ++j) {                      // hsu(), in place
      const uint64_t old = row_of(row, j);
      if (old == 0) continue;                          // wave-uniform: nothing to clear
      const bool self = (old >> j) & 1ull;
      if (lane == j) {
        if (self) row = 0;
      } else if (((row >> j) & 1ull) && (lane < j || !self)) {
        row &= ~old;
      }
    }
    if (G.keep) row |= m;                              // p_keep = 1: every listed edge stays (graphs_utils.py:79-80)
    M[p][lane] = row;
    const int inc = wave_incscan(__popcll(row), lane);
    if (lane == 63) out_n[p] = inc;
  }
  __syncthreads();

  // ---- offsets: predicates in the order of their first listed row
  if (tid < P) {
    int at = 0;
    for (int q = 0; q < P; ++q)
      if (first[q] < first[tid]) at += out_n[q];
    base[tid] = at;
  }
  if (tid == 0) {
    int sum = 0;
    for (int q = 0; q < P; ++q) sum += out_n[q];
    total = sum;
  }
  __syncthreads();
  const int n_rel = total;

  if (!EMIT) {
    if (tid == 0) counts[b] = bad ? -1 - (int64_t)(n_rel + n) : (int64_t)(n_rel + n);   // negative: a device row was refused
    return;
  }
  int64_t* trip = triplets + (int64_t)b * T * 3;
  int64_t* tt = ttype + (int64_t)b * T;
  if (!bad) {
    for (int p = wave; p < P; p += GNW) {
      const int c = listed[p];
      if (c == 0) continue;
      if (c < 3) {
        if (lane < c) {
          const int r = lane == 0 ? first[p] : last[p];
          put(trip, tt, base[p] + lane, T, rows[r * 3 + 0], p, rows[r * 3 + 2]);
        }
        continue;
      }
      uint64_t row = M[p][lane];
      const int cnt = __popcll(row);
      int64_t at = base[p] + (wave_incscan(cnt, lane) - cnt);
      while (row) {                                    // matrix_to_triplets: np.where's row-major order
        const int o = __ffsll((long long)row) - 1;
        row &= row - 1;
        put(trip, tt, at++, T, lane, p, o);
      }
    }
    if (tid < n) put(trip, tt, n_rel + tid, T, tid, G.pid_in_image, n);          // clevr_dialog.py:301-304
  }
  for (int64_t t = (bad ? 0 : n_rel + n) + tid; t < T; t += GNT) put(trip, tt, t, T, 0, G.pid_padding, 0);   // :447-451
}

int check_common(const char* fn, int64_t B, int64_t O, int64_t R, int64_t P, int64_t pid_padding, int64_t pid_in_image,
                 int keep) {
  CSG_REQUIRE(B > 0 && B < (1ll << 31) && O > 0 && O < (1ll << 31) && R >= 0 && R < (1ll << 31) / 3 && P > 0, CSG_E_BADSHAPE,
              "%s: bad shape B=%ld O=%ld R=%ld P=%ld", fn, (long)B, (long)O, (long)R, (long)P);
  CSG_REQUIRE(P <= GMAXP, CSG_E_UNSUPPORTED, "%s: at most %d predicates (got %ld)", fn, GMAXP, (long)P);
  CSG_REQUIRE(pid_padding >= 0 && pid_padding < P && pid_in_image >= 0 && pid_in_image < P && pid_padding != pid_in_image,
              CSG_E_BADSHAPE, "%s: __padding__ = %ld and __in_image__ = %ld must be two ids of [0, %ld)", fn, (long)pid_padding,
              (long)pid_in_image, (long)P);
  CSG_REQUIRE(keep == 0 || keep == 1, CSG_E_BADSHAPE, "%s: keep (use_transitivity) must be 0 or 1 (got %d)", fn, keep);
  return CSG_OK;
}

GraphParams params(int64_t O, int64_t R, int64_t P, int64_t pid_padding, int64_t pid_in_image, int keep) {
  GraphParams G;
  G.P = (int)P;
  G.O = (int)O;
  G.R = (int)R;
  G.pid_padding = (int)pid_padding;
  G.pid_in_image = (int)pid_in_image;
  G.keep = keep;
  return G;
}

}  // namespace

extern "C" {

int csg_clevr_graph_count(const int64_t* n_rows, const int64_t* n_rows_host, int64_t B, int64_t O, const int64_t* rel,
                          const int64_t* rel_host, int64_t R, int64_t P, int64_t pid_padding, int64_t pid_in_image, int keep,
                          int64_t* counts, void* stream) {
  const int rc = check_common("csg_clevr_graph_count", B, O, R, P, pid_padding, pid_in_image, keep);
  if (rc != CSG_OK) return rc;
  CSG_REQUIRE(n_rows && n_rows_host && counts && (R == 0 || (rel && rel_host)), CSG_E_BADSHAPE,
              "csg_clevr_graph_count: null argument");
  CSG_REQUIRE(((uintptr_t)rel & 7) == 0, CSG_E_BADSHAPE, "csg_clevr_graph_count: rel must be 8-byte aligned");
  // every input the host holds is checked here, before anything is enqueued
  for (int64_t b = 0; b < B; ++b) {
    const int64_t rows = n_rows_host[b];
    CSG_REQUIRE(rows >= 1 && rows <= O, CSG_E_BADSHAPE,
                "csg_clevr_graph_count: n_objs[%ld] = %ld outside [1, %ld] (a sample has its __image__ row)", (long)b,
                (long)rows, (long)O);
    CSG_REQUIRE(rows <= GMAXN, CSG_E_UNSUPPORTED,
                "csg_clevr_graph_count: at most %d objects per sample, %d rows with the __image__ row (sample %ld has %ld rows)",
                GMAXN - 1, GMAXN, (long)b, (long)rows);
    const int64_t n = rows - 1;
    for (int64_t r = 0; r < R; ++r) {
      const int64_t* t = rel_host + (b * R + r) * 3;
      const int64_t s = t[0], p = t[1], o = t[2];
      if (p == pid_padding) continue;
      CSG_REQUIRE(p >= 0 && p < P, CSG_E_BADSHAPE, "csg_clevr_graph_count: sample %ld row %ld: predicate %ld outside [0, %ld)",
                  (long)b, (long)r, (long)p, (long)P);
      CSG_REQUIRE(s >= 0 && s < n && o >= 0 && o < n, CSG_E_BADSHAPE,
                  "csg_clevr_graph_count: sample %ld row %ld: object %ld or %ld outside [0, %ld)", (long)b, (long)r, (long)s,
                  (long)o, (long)n);
    }
  }
  hipStream_t st = (hipStream_t)stream;
  ProfScope pr(K_CLEVR_GRAPH_COUNT, (double)B * (R + P * GMAXN), st);
  CSG_LAUNCH(k_clevr_graph<false>, dim3((unsigned)B), dim3(GNT), 0, st, params(O, R, P, pid_padding, pid_in_image, keep), n_rows,
             rel, counts, (int64_t)0, (int64_t*)nullptr, (int64_t*)nullptr);
  return check_launch("csg_clevr_graph_count");
}

int csg_clevr_graph_emit(const int64_t* n_rows, int64_t B, int64_t O, const int64_t* rel, int64_t R, int64_t P,
                         int64_t pid_padding, int64_t pid_in_image, int keep, int64_t T, int64_t* triplets,
                         int64_t* triplet_type, void* stream) {
  const int rc = check_common("csg_clevr_graph_emit", B, O, R, P, pid_padding, pid_in_image, keep);
  if (rc != CSG_OK) return rc;
  CSG_REQUIRE(T >= 0 && T < (1ll << 31) && n_rows && (R == 0 || rel), CSG_E_BADSHAPE,
              "csg_clevr_graph_emit: bad shape T=%ld or null argument", (long)T);
  CSG_REQUIRE(((uintptr_t)rel & 7) == 0, CSG_E_BADSHAPE, "csg_clevr_graph_emit: rel must be 8-byte aligned");
  if (T == 0) return CSG_OK;
  CSG_REQUIRE(triplets && triplet_type, CSG_E_BADSHAPE, "csg_clevr_graph_emit: null argument");
  hipStream_t st = (hipStream_t)stream;
  ProfScope pr(K_CLEVR_GRAPH_EMIT, (double)B * T * 32, st);
  CSG_LAUNCH(k_clevr_graph<true>, dim3((unsigned)B), dim3(GNT), 0, st, params(O, R, P, pid_padding, pid_in_image, keep), n_rows,
             rel, (int64_t*)nullptr, T, triplets, triplet_type);
  return check_launch("csg_clevr_graph_emit");
}

}  // extern "C"
