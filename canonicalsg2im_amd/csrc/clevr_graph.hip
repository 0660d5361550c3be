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
#include "csg_bitgraph.h"

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
    uint64_t row = wave_close(m, n, lane);             // path()
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
  int64_t* tt = ttype + (int64_t)b * T;                // every row is an ORIGINAL_EDGE = 0, the padding too
  if (!bad) {
    for (int p = wave; p < P; p += GNW) {
      const int c = listed[p];
      if (c == 0) continue;
      if (c < 3) {
        if (lane < c) {
          const int r = lane == 0 ? first[p] : last[p];
          put_triplet(trip, tt, base[p] + lane, T, rows[r * 3 + 0], p, rows[r * 3 + 2], 0);
        }
        continue;
      }
      const uint64_t row = M[p][lane];
      const int cnt = __popcll(row);                   // matrix_to_triplets: np.where's row-major order
      emit_bits(row, 0, base[p] + (wave_incscan(cnt, lane) - cnt), T, trip, tt, lane, p, 0);
    }
    if (tid < n) put_triplet(trip, tt, n_rel + tid, T, tid, G.pid_in_image, n, 0);          // clevr_dialog.py:301-304
  }
  for (int64_t t = (bad ? 0 : n_rel + n) + tid; t < T; t += GNT) put_triplet(trip, tt, t, T, 0, G.pid_padding, 0, 0);   // :447-451
}

int check_common(const char* fn, int64_t B, int64_t O, int64_t R, int64_t P, int64_t pid_padding, int64_t pid_in_image,
                 int keep) {
  CSG_REQUIRE(B > 0 && B < (1ll << 31) && O > 0 && O < (1ll << 31) && R >= 0 && R < (1ll << 31) / 3 && P > 0, CSG_E_BADSHAPE,
              "%s: bad shape B=%ld O=%ld R=%ld P=%ld", fn, (long)B, (long)O, (long)R, (long)P);
  CSG_REQUIRE(P <= GMAXP, CSG_E_UNSUPPORTED, "%s: at most %d predicates (got %ld)", fn, GMAXP, (long)P);
  if (const int rc = check_meta_ids(fn, P, pid_padding, pid_in_image)) return rc;
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
      const int rc = check_host_row("csg_clevr_graph_count", true, "", rel_host + (b * R + r) * 3, b, r, P, pid_padding, n);
      if (rc < 0) return rc;
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
