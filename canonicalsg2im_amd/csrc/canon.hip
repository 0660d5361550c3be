// Canonical scene-graph construction of the packed datasets, on the device.
//
// Reference (numpy / python loops, O(O^3) per sample, ~2.5 s per graph at O = 128):
//   BaseDataset.add_location_triplets   sg2im/data/base_dataset.py:35-87
//   triplets_to_minimal / path / hsu    scripts/graphs_utils.py:15-71
//   BaseDataset.add_dummy_triplets      sg2im/data/base_dataset.py:141-151
//   BaseDataset.add_learnt_triplets     sg2im/data/base_dataset.py:89-139
//   get_edge_converse_triplets          scripts/graphs_utils.py:126-152 (learned_converse = 1: k_canon_converse)
//   get_current_and_transitive_triplets scripts/graphs_utils.py:96-100
//   triplet padding of the collate      sg2im/data/packed_clevr_dialog.py:309-315
//
// One workgroup per sample.  The six location relations are 256x256 bit matrices in LDS (one
// 64-bit word = 64 objects of a row): the pair loop sets bits, Warshall's closure ORs whole rows
// (one barrier per pivot), Hsu's reduction clears them with AND-NOT in the reference's pivot order.
// Integer/bit work end to end: results are bit-identical to the reference's.  Emission order is
// the one np.unique(axis=0) produces — (s, p, o) lexicographic — followed by the transitive extras
// in (ascending predicate id, s, o) order.
//
// Further down: the same pipeline per (sample, predicate) for annotated rows and any vocabulary (csg_canon_general_*), and
// for the unpacked COCO dataset's sampled pairs (sg2im/data/coco.py:365-428) k_pair_relations, which gives each drawn pair
// its predicate, and k_gen_pack, which takes such device rows into that pipeline (csg_canon_general_build_dev).
// This file is NOT compiled with -ffp-contract=off; k_pair_relations, the one kernel here that adds to a product, turns
// contraction off for itself.
#include "csg_bitgraph.h"

#include <vector>

using namespace csg;

namespace {

constexpr int MAXN = 256;        // objects per sample (incl. the __image__ object)
constexpr int W = MAXN / 64;     // 64-bit words per bit-matrix row
constexpr int NREL = 6;          // __below__ __above__ __left of__ __right of__ __inside__ __surrounding__

struct CanonParams {
  int O;                  // padded objects per sample in the input tensors
  int image_id;           // id of the __image__ object (first attribute)
  int pid[NREL];          // predicate id of each location relation, in the order above
  int pid_in_image;       // predicate id of __in_image__
  int pid_padding;        // predicate id of __padding__
  int order[NREL + 1];    // relation slots (0..5, 6 = __in_image__) sorted by ascending predicate id
  int include_dummies;
  int learned_transitivity;
};

// workspace per sample: R[NREL][MAXN][W] | X[NREL][MAXN][W] (u64) | off_orig[MAXN] | off_trans[NREL][MAXN] (i32)
constexpr int64_t kBitWords = (int64_t)NREL * MAXN * W;
constexpr int64_t kWsBytesPerSample = 2 * kBitWords * 8 + (int64_t)(MAXN + NREL * MAXN) * 4;

__device__ __forceinline__ uint64_t* ws_R(void* ws, int b) { return (uint64_t*)((char*)ws + (int64_t)b * kWsBytesPerSample); }
__device__ __forceinline__ uint64_t* ws_X(void* ws, int b) { return ws_R(ws, b) + kBitWords; }
__device__ __forceinline__ int* ws_off(void* ws, int b) { return (int*)(ws_X(ws, b) + kBitWords); }

// exclusive scan of one int per thread over the 256-thread block; returns the block total in *total
__device__ int block_exscan(int v, int* sm, int* total) {
  const int tid = threadIdx.x;
  __syncthreads();
  sm[tid] = v;
  __syncthreads();
  for (int o = 1; o < 256; o <<= 1) {
    int t = tid >= o ? sm[tid - o] : 0;
    __syncthreads();
    sm[tid] += t;
    __syncthreads();
  }
  *total = sm[255];
  return sm[tid] - v;
}

// objects of sample b: never more than the input tensors or a bit matrix hold
__device__ __forceinline__ int canon_n(const CanonParams& P, const int64_t* __restrict__ n_objs, int b) {
  int n = (int)n_objs[b];
  if (n > P.O) n = P.O;
  if (n > MAXN) n = MAXN;
  return n;
}

// the index of the sample's first row that carries P.image_id among `ids` (objs0's row of the sample), or -1; every
// thread of the block calls it
__device__ __forceinline__ int image_row(const int64_t* __restrict__ ids, int64_t image_id, int n, int* sm) {
  const int tid = threadIdx.x;
  sm[tid] = (tid < n && ids[tid] == image_id) ? tid : MAXN;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (tid < o) sm[tid] = min(sm[tid], sm[tid + o]);
    __syncthreads();
  }
  return sm[0] < MAXN ? sm[0] : -1;
}

// path(): Warshall closure of the six matrices, pivot i (graphs_utils.py:15-27); one barrier per pivot and one after
__device__ __forceinline__ void close_relations(uint64_t (&adj)[NREL][MAXN][W], int n) {
  const int tid = threadIdx.x, nw = (n + 63) >> 6, tasks = NREL * n;
  for (int i = 0; i < n; ++i) {
    __syncthreads();
    for (int t = tid; t < tasks; t += 256) {
      const int r = t / n, j = t - r * n;
      if (j != i && ((adj[r][j][i >> 6] >> (i & 63)) & 1ull)) {
        for (int w = 0; w < nw; ++w) adj[r][j][w] |= adj[r][i][w];
      }
    }
  }
  __syncthreads();
}

// Per-row counts -> offsets, and the sample's two counts.  `cur` [NREL][MAXN][W]: the current graphs, in LDS or the
// workspace's R; X: the workspace's extras.  Both as the whole block sees them.
__device__ __forceinline__ void counts_and_offsets(const CanonParams& P, const int64_t* __restrict__ objs0, int b, int n,
                                                   const uint64_t* cur, const uint64_t* X, int* off, int* scan,
                                                   int64_t* __restrict__ counts) {
  const int tid = threadIdx.x, nw = (n + 63) >> 6;
  // the __image__ object's index (base_dataset.py:144)
  const int img = P.include_dummies ? image_row(objs0 + (int64_t)b * P.O, (int64_t)P.image_id, n, scan) : -1;
  int c = 0;
  if (tid < n) {
    for (int r = 0; r < NREL; ++r)
      for (int w = 0; w < nw; ++w) c += __popcll(cur[((int64_t)r * MAXN + tid) * W + w]);
    if (img >= 0 && tid != img) c += 1;
  }
  int total = 0;
  int ex = block_exscan(c, scan, &total);
  off[tid] = ex;
  const int n_orig = total;
  int n_trans = 0;
  if (P.learned_transitivity) {
    for (int q = 0; q < NREL + 1; ++q) {               // extras per relation, in predicate order
      const int r = P.order[q];
      if (r >= NREL) continue;
      int cx = 0;
      if (tid < n)
        for (int w = 0; w < nw; ++w) cx += __popcll(X[((int64_t)r * MAXN + tid) * W + w]);
      int tot = 0;
      int e = block_exscan(cx, scan, &tot);
      off[MAXN + r * MAXN + tid] = n_trans + e;
      n_trans += tot;
    }
  }
  if (tid == 0) {
    counts[b * 2 + 0] = n_orig;
    counts[b * 2 + 1] = n_trans;
  }
}

__global__ __launch_bounds__(256) void k_canon_build(CanonParams P, const int64_t* __restrict__ objs0,
                                                      const float* __restrict__ boxes,
                                                      const float* __restrict__ centers,
                                                      const int64_t* __restrict__ n_objs, void* __restrict__ ws,
                                                      int64_t* __restrict__ counts) {
  __shared__ uint64_t adj[NREL][MAXN][W];      // 48 KB
  __shared__ float gx0[MAXN], gy0[MAXN], gxc[MAXN], gyc[MAXN], gcx[MAXN], gcy[MAXN];
  __shared__ int real[MAXN];
  __shared__ int scan[256];
  const int b = blockIdx.x, tid = threadIdx.x;
  const int n = canon_n(P, n_objs, b), nw = (n + 63) >> 6;

  for (int i = tid; i < NREL * MAXN * W; i += 256) (&adj[0][0][0])[i] = 0;
  if (tid < MAXN) {
    int r = 0;
    float x0 = 0.f, y0 = 0.f, xc = 0.f, yc = 0.f, cx = 0.f, cy = 0.f;
    if (tid < n) {
      const float* bx = boxes + ((int64_t)b * P.O + tid) * 4;
      x0 = bx[0];
      y0 = bx[1];
      xc = __fadd_rn(x0, bx[2] * 0.5f);          // `sx1 = sx0 + sw / 2` (base_dataset.py:47): the box CENTRE, fp32
      yc = __fadd_rn(y0, bx[3] * 0.5f);
      cx = centers[((int64_t)b * P.O + tid) * 2 + 0];
      cy = centers[((int64_t)b * P.O + tid) * 2 + 1];
      r = (n > 1) && (objs0[(int64_t)b * P.O + tid] != (int64_t)P.image_id);   // base_dataset.py:39-41
    }
    gx0[tid] = x0; gy0[tid] = y0; gxc[tid] = xc; gyc[tid] = yc; gcx[tid] = cx; gcy[tid] = cy;
    real[tid] = r;
  }
  __syncthreads();

  // ---- pair loop (base_dataset.py:42-81): thread s builds row s of the six matrices
  if (tid < n && real[tid]) {
    const int s = tid;
    const float sx0 = gx0[s], sy0 = gy0[s], sxc = gxc[s], syc = gyc[s], scx = gcx[s], scy = gcy[s];
    for (int w = 0; w < nw; ++w) {
      uint64_t m[NREL] = {0, 0, 0, 0, 0, 0};
      const int hi = min(64, n - w * 64);
      for (int k = 0; k < hi; ++k) {
        const int o = w * 64 + k;
        if (o == s || !real[o]) continue;
        const uint64_t bit = 1ull << k;
        const float ox0 = gx0[o], oy0 = gy0[o], oxc = gxc[o], oyc = gyc[o];
        if (sx0 < ox0 && sxc > oxc && sy0 < oy0 && syc > oyc) {
          m[5] |= bit;                                            // __surrounding__
        } else if (sx0 > ox0 && sxc < oxc && sy0 > oy0 && syc < oyc) {
          m[4] |= bit;                                            // __inside__
        } else {
          // d = obj_centers[s] - obj_centers[o]; the sign of an IEEE difference is the comparison
          const float ocx = gcx[o], ocy = gcy[o];
          if (scx > ocx) m[3] |= bit; else if (scx < ocx) m[2] |= bit;      // __right of__ / __left of__
          if (scy > ocy) m[0] |= bit; else if (scy < ocy) m[1] |= bit;      // __below__ / __above__
        }
      }
      for (int r = 0; r < NREL; ++r) adj[r][s][w] = m[r];
    }
  }

  close_relations(adj, n);
  const int tasks = NREL * n;
  uint64_t* X = ws_X(ws, b);
  uint64_t* R = ws_R(ws, b);
  for (int t = tid; t < tasks * W; t += 256) {       // park the closure in X
    const int w = t % W, rj = t / W;
    const int r = rj / n, j = rj - r * n;
    X[((int64_t)r * MAXN + j) * W + w] = adj[r][j][w];
  }

  // ---- hsu(): reduction in the reference's pivot order j (graphs_utils.py:30-38).  The location
  // relations are strict orders, so m[j][j] is never set and row j is not written while it is read.
  for (int j = 0; j < n; ++j) {
    __syncthreads();
    for (int t = tid; t < tasks; t += 256) {
      const int r = t / n, i = t - r * n;
      if (i != j && ((adj[r][i][j >> 6] >> (j & 63)) & 1ull)) {
        for (int w = 0; w < nw; ++w) adj[r][i][w] &= ~adj[r][j][w];
      }
    }
  }
  __syncthreads();
  for (int t = tid; t < tasks * W; t += 256) {
    const int w = t % W, rj = t / W;
    const int r = rj / n, j = rj - r * n;
    const int64_t at = ((int64_t)r * MAXN + j) * W + w;
    const uint64_t red = adj[r][j][w];
    R[at] = red;
    X[at] = X[at] & ~red;                             // closure - current (graphs_utils.py:96-100)
  }

  counts_and_offsets(P, objs0, b, n, &adj[0][0][0], X, ws_off(ws, b), scan, counts);     // adj = R, still in LDS
}

__global__ __launch_bounds__(256) void k_canon_emit(CanonParams P, const int64_t* __restrict__ objs0,
                                                     const int64_t* __restrict__ n_objs,
                                                     const void* __restrict__ ws, const int64_t* __restrict__ counts,
                                                     int64_t T, int64_t* __restrict__ triplets,
                                                     int64_t* __restrict__ ttype) {
  __shared__ int red[256];
  const int b = blockIdx.x, tid = threadIdx.x;
  const int n = canon_n(P, n_objs, b), nw = (n + 63) >> 6;
  const uint64_t* R = ws_R((void*)ws, b);
  const uint64_t* X = ws_X((void*)ws, b);
  const int* off = ws_off((void*)ws, b);
  int64_t* trip = triplets + (int64_t)b * T * 3;
  int64_t* tt = ttype + (int64_t)b * T;
  const int n_orig = (int)counts[b * 2 + 0], n_trans = (int)counts[b * 2 + 1];

  const int img = P.include_dummies ? image_row(objs0 + (int64_t)b * P.O, (int64_t)P.image_id, n, red) : -1;
  if (tid < n) {
    const int s = tid;
    int64_t at = off[s];
    for (int q = 0; q < NREL + 1; ++q) {               // ascending predicate id: np.unique's (s, p, o) order
      const int r = P.order[q];
      if (r >= NREL) {
        if (img >= 0 && s != img) put_triplet(trip, tt, at++, T, s, P.pid_in_image, img, 0);
        continue;
      }
      for (int w = 0; w < nw; ++w) at = emit_bits(R[((int64_t)r * MAXN + s) * W + w], w * 64, at, T, trip, tt, s, P.pid[r], 0);
    }
    if (n_trans) {
      for (int q = 0; q < NREL + 1; ++q) {
        const int r = P.order[q];
        if (r >= NREL) continue;
        int64_t a2 = (int64_t)n_orig + off[MAXN + r * MAXN + s];
        for (int w = 0; w < nw; ++w) a2 = emit_bits(X[((int64_t)r * MAXN + s) * W + w], w * 64, a2, T, trip, tt, s, P.pid[r], 1);
      }
    }
  }
  for (int64_t t = (int64_t)n_orig + n_trans + tid; t < T; t += 256)      // packed_clevr_dialog.py:309-315
    put_triplet(trip, tt, t, T, 0, P.pid_padding, 0, 0);
}


// ---- learned_converse = 1 (base_dataset.py:104-107, graphs_utils.py:126-152).  For every original triplet (s, rel, o) of
// the six location relations — in the reference's order: relations by ascending predicate id, triplets by (s, o) — ONE
// uniform number u decides through the relation's cumulative distribution whether a converse edge (o, r, s) is added and
// for which other relation r.  The distribution (scipy softmax over the five candidate weights and a zero for "none",
// numpy's cumsum / normalisation in float64) is computed on the host exactly as numpy.random.choice does and arrives as
// `cdf` (6 relations x 6 thresholds); the uniforms are the host's np.random stream (the reference's global RNG), one per
// triplet, `u_off[b]` = the number of triplets of the samples before b.  The choice is searchsorted(cdf, u, 'right'): the
// number of thresholds <= u.  Converse edges join their relation BEFORE the transitive closure is taken (:109-120), so the
// closure, the "current" graph and every count are recomputed here: R <- minimal + converse, X <- closure(R) - R (the
// diagonal included: converse edges can close cycles, and `path` then marks i -> i), conv_counts[rel][r] += 1 per draw.
__global__ __launch_bounds__(256) void k_canon_converse(CanonParams P, const int64_t* __restrict__ objs0,
                                                         const int64_t* __restrict__ n_objs, void* __restrict__ ws,
                                                         const double* __restrict__ cdf, const double* __restrict__ uniforms,
                                                         const int64_t* __restrict__ u_off, int npred,
                                                         float* __restrict__ conv_counts, int64_t* __restrict__ counts) {
  __shared__ uint64_t adj[NREL][MAXN][W];      // converse edges first, then R | converse, then its closure
  __shared__ int scan[256];
  __shared__ int hist[NREL][NREL];             // [relation slot][choice 0..4 = candidate, 5 = none]
  __shared__ int cand[NREL][NREL - 1];         // candidate relation slots of a slot, ascending predicate id
  const int b = blockIdx.x, tid = threadIdx.x;
  const int n = canon_n(P, n_objs, b), nw = (n + 63) >> 6;
  uint64_t* R = ws_R(ws, b);
  uint64_t* X = ws_X(ws, b);
  for (int i = tid; i < NREL * MAXN * W; i += 256) (&adj[0][0][0])[i] = 0;
  if (tid < NREL * NREL) (&hist[0][0])[tid] = 0;
  if (tid < NREL) {
    int k = 0;
    for (int q = 0; q < NREL + 1; ++q) {
      const int r = P.order[q];
      if (r < NREL && r != tid) cand[tid][k++] = r;
    }
  }
  __syncthreads();
  // ---- one draw per original triplet, numbered in (relation by ascending id, s, o) order
  int base = 0;
  for (int q = 0; q < NREL + 1; ++q) {
    const int r = P.order[q];
    if (r >= NREL) continue;
    int c = 0;
    if (tid < n)
      for (int w = 0; w < nw; ++w) c += __popcll(R[((int64_t)r * MAXN + tid) * W + w]);
    int tot = 0;
    int k = base + block_exscan(c, scan, &tot);
    if (tid < n) {
      const int s = tid;
      const double* cd = cdf + r * NREL;
      for (int w = 0; w < nw; ++w) {
        uint64_t m = R[((int64_t)r * MAXN + s) * W + w];
        while (m) {
          const int o = w * 64 + pop_bit(m);
          const double u = uniforms[u_off[b] + k];
          ++k;
          const int j = choice_right(cd, NREL, u);
          atomicAdd(&hist[r][j], 1);
          if (j < NREL - 1)                                    // converse edge (o, cand, s)
            atomicOr((unsigned long long*)&adj[cand[r][j]][o][s >> 6], 1ull << (s & 63));
        }
      }
    }
    base += tot;
  }
  __syncthreads();
  // ---- R <- minimal | converse (np.unique removes a converse edge that repeats an original one)
  const int tasks = NREL * n;
  for (int t = tid; t < tasks * W; t += 256) {
    const int w = t % W, rj = t / W;
    const int r = rj / n, j = rj - r * n;
    const int64_t at = ((int64_t)r * MAXN + j) * W + w;
    const uint64_t v = adj[r][j][w] | R[at];
    adj[r][j][w] = v;
    R[at] = v;
  }
  // ---- closure of the new graphs (path(): graphs_utils.py:15-27), X <- closure - current
  if (P.learned_transitivity) {
    close_relations(adj, n);
    for (int t = tid; t < tasks * W; t += 256) {
      const int w = t % W, rj = t / W;
      const int r = rj / n, j = rj - r * n;
      const int64_t at = ((int64_t)r * MAXN + j) * W + w;
      X[at] = adj[r][j][w] & ~R[at];
    }
  }
  __syncthreads();
  counts_and_offsets(P, objs0, b, n, R, X, ws_off(ws, b), scan, counts);
  // ---- conv_counts[b][rel][r] (base_dataset.py:93, graphs_utils.py:146): r = a relation id, or npred for "none"
  if (tid < NREL * NREL) {
    const int r = tid / NREL, j = tid - r * NREL;
    const int col = j < NREL - 1 ? P.pid[cand[r][j]] : npred;
    conv_counts[((int64_t)b * npred + P.pid[r]) * (npred + 1) + col] = (float)hist[r][j];
  }
}

int fill_params(CanonParams* P, int64_t O, const int32_t* pred_ids, int64_t image_id, int include_dummies,
                int learned_transitivity) {
  P->O = (int)O;
  P->image_id = (int)image_id;
  P->pid_padding = pred_ids[0];
  P->pid_in_image = pred_ids[1];
  for (int r = 0; r < NREL; ++r) P->pid[r] = pred_ids[2 + r];
  int key[NREL + 1];
  for (int r = 0; r < NREL; ++r) key[r] = P->pid[r];
  key[NREL] = P->pid_in_image;
  for (int q = 0; q < NREL + 1; ++q) P->order[q] = q;
  for (int a = 1; a < NREL + 1; ++a)            // insertion sort by predicate id
    for (int c = a; c > 0 && key[P->order[c]] < key[P->order[c - 1]]; --c) {
      int t = P->order[c];
      P->order[c] = P->order[c - 1];
      P->order[c - 1] = t;
    }
  for (int a = 0; a < NREL + 1; ++a)
    for (int c = a + 1; c < NREL + 1; ++c)
      if (key[a] == key[c] || key[a] == P->pid_padding) return 0;
  P->include_dummies = include_dummies;
  P->learned_transitivity = learned_transitivity;
  return 1;
}


// ==== annotated relationships and any vocabulary (packed_vg.py:127-142) ==========================================
// The graph of a sample is cut per (sample, predicate): one 256x256 bit matrix of a predicate fits LDS, the 44+ of a
// Visual Genome vocabulary do not.  Phases that need another block's results are separate launches:
//   geometry   k_canon_build (above) on the six location relations alone: their per-relation minimal graphs
//   scatter    (sample, predicate): U = annotated rows | geometric minimal graph | __in_image__ dummies  (np.unique)
//   draws      (sample): the prefix count of original rows over the non-meta predicates by ascending id
//   converse   (sample, predicate): one uniform per row of U, in (s, o) order; converse edges OR-ed into V of the chosen
//              predicate (integer atomics)
//   close      (sample, predicate): U <- U | V; Warshall on U; V <- closure - U; per-row counts
//   offsets    (sample): per-row counts -> output positions, (s, p, o) for the originals, (p, s, o) for the extras
//   emit       (sample, predicate): the rows of U and V at those positions, then the collate's padding
constexpr int GMAXP = 256;       // predicates of a vocabulary

struct GenParams {
  int B, P, O;
  int K;                         // non-meta predicates; a draw chooses among K - 1 candidates and "none"
  int image_id;
  int pid_padding, pid_in_image;
  int include_dummies, learned_transitivity;
  signed char role[GMAXP];       // CSG_CANON_ROLE_*, or the location slot 0..5
  unsigned char nm[GMAXP];       // the non-meta predicate ids, ascending
  unsigned char rank[GMAXP];     // position of a non-meta predicate in nm
};

struct GenWs {
  uint64_t* U;                   // [B][P][MAXN][W] original rows of a predicate
  uint64_t* V;                   // [B][P][MAXN][W] converse edges drawn into it, then its transitive extras
  int* rc;                       // [B][P][MAXN] originals per row -> their first output position
  int* xc;                       // [B][P][MAXN] extras per row -> their first output position
  int* tot;                      // [B][P][2] originals (after scatter, then after close), extras
  int* flag;                     // [B][P] converse edges were drawn into the predicate
  int* doff;                     // [B][P] first draw of the predicate's rows within the sample
  int64_t* geo_counts;           // [B][2] k_canon_build's counts (unused)
  int* bad;                      // [B] a row given on the device was dropped (csg_canon_general_build_dev); else 0
  int64_t* nob;                  // [B] objects per sample
  int* rbeg;                     // [B + 1] first annotated row of a sample
  uint32_t* rows;                // annotated rows: s | o << 8 | p << 16
};

__host__ __device__ inline int64_t gen_align(int64_t x) { return (x + 255) & ~(int64_t)255; }

// byte offsets of the regions; the annotated rows come last, so every region but them depends on (B, P) only
inline int64_t gen_layout(int64_t B, int64_t P, int64_t R, void* base, GenWs* w) {
  char* b = (char*)base;
  int64_t at = gen_align(B * kWsBytesPerSample);
  const int64_t mat = B * P * MAXN * W * 8, row = B * P * MAXN * 4;
  if (w) {
    w->U = (uint64_t*)(b + at);
    w->V = (uint64_t*)(b + at + mat);
  }
  at += 2 * mat;
  if (w) {
    w->rc = (int*)(b + at);
    w->xc = (int*)(b + at + row);
  }
  at += 2 * row;
  if (w) w->tot = (int*)(b + at);
  at += gen_align(B * P * 2 * 4);
  if (w) w->flag = (int*)(b + at);
  at += gen_align(B * P * 4);
  if (w) w->doff = (int*)(b + at);
  at += gen_align(B * P * 4);
  if (w) w->geo_counts = (int64_t*)(b + at);
  at += gen_align(B * 2 * 8);
  if (w) w->bad = (int*)(b + at);
  at += gen_align(B * 4);
  if (w) w->nob = (int64_t*)(b + at);
  at += gen_align(B * 8);
  if (w) w->rbeg = (int*)(b + at);
  at += gen_align((B + 1) * 4);
  if (w) w->rows = (uint32_t*)(b + at);
  at += gen_align(B * R * 4);
  return at;
}

__device__ __forceinline__ int gen_n(const GenWs& w, const GenParams& P, int b) {
  int n = (int)w.nob[b];
  return n > MAXN ? MAXN : n;
}

__device__ __forceinline__ int block_sum(int v, int* sm) {
  int total = 0;
  (void)block_exscan(v, sm, &total);
  return total;
}

// ---- scatter: U[b][p] = annotated rows of p | the geometric minimal graph (location slots) | the dummies (__in_image__)
__global__ __launch_bounds__(256) void k_gen_scatter(GenParams P, const int64_t* __restrict__ objs0, GenWs w, void* geo) {
  __shared__ uint64_t adj[MAXN][W];
  __shared__ int scan[256];
  const int p = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
  const int n = gen_n(w, P, b), nw = (n + 63) >> 6;
  const int role = P.role[p];
  for (int i = tid; i < n * W; i += 256) (&adj[0][0])[i] = 0;
  const int img = (role == CSG_CANON_ROLE_IN_IMAGE && P.include_dummies)      // base_dataset.py:141-151
                      ? image_row(objs0 + (int64_t)b * P.O, (int64_t)P.image_id, n, scan) : -1;
  __syncthreads();
  if (tid < n) {
    if (role >= 0 && geo != nullptr) {                                // base_dataset.py:83-87; no geometry: authored rows alone
      const uint64_t* Rg = ws_R(geo, b) + ((int64_t)role * MAXN + tid) * W;
      for (int k = 0; k < nw; ++k) adj[tid][k] = Rg[k];
    }
    if (img >= 0 && tid != img) adj[tid][img >> 6] |= 1ull << (img & 63);
  }
  __syncthreads();
  const int r0 = w.rbeg[b], r1 = w.rbeg[b + 1];
  for (int r = r0 + tid; r < r1; r += 256) {                          // packed_vg.py:127-138
    const uint32_t v = w.rows[r];
    if ((int)(v >> 16) != p) continue;
    const int s = v & 255, o = (v >> 8) & 255;
    atomicOr((unsigned long long*)&adj[s][o >> 6], 1ull << (o & 63));
  }
  __syncthreads();
  int c = 0;
  if (tid < n) {
    const int64_t at = (((int64_t)b * P.P + p) * MAXN + tid) * W;
    for (int k = 0; k < nw; ++k) {
      const uint64_t m = adj[tid][k];
      w.U[at + k] = m;
      w.V[at + k] = 0;
      c += __popcll(m);
    }
  }
  const int total = block_sum(c, scan);
  if (tid == 0) {
    w.tot[((int64_t)b * P.P + p) * 2 + 0] = total;
    w.tot[((int64_t)b * P.P + p) * 2 + 1] = 0;
    w.flag[(int64_t)b * P.P + p] = 0;
  }
}

// ---- draws: the first draw of each non-meta predicate's rows (predicates by ascending id); counts[b] = {draws, 0}
__global__ __launch_bounds__(256) void k_gen_draws(GenParams P, GenWs w, int64_t* __restrict__ counts) {
  __shared__ int scan[256];
  const int b = blockIdx.x, tid = threadIdx.x;
  const int c = (tid < P.P && P.role[tid] != CSG_CANON_ROLE_PADDING && P.role[tid] != CSG_CANON_ROLE_IN_IMAGE)
                    ? w.tot[((int64_t)b * P.P + tid) * 2] : 0;
  int total = 0;
  const int ex = block_exscan(c, scan, &total);
  if (tid < P.P) w.doff[(int64_t)b * P.P + tid] = ex;
  if (tid == 0) {
    counts[b * 2 + 0] = w.bad[b] ? -1 - (int64_t)total : total;      // negative: a device row was refused
    counts[b * 2 + 1] = 0;
  }
}

// ---- converse (base_dataset.py:104-107, graphs_utils.py:126-152): block (rel, b) draws for the rows of U[b][rel]
__global__ __launch_bounds__(256) void k_gen_converse(GenParams P, GenWs w, const double* __restrict__ cdf,
                                                      const double* __restrict__ uniforms, const int64_t* __restrict__ u_off,
                                                      float* __restrict__ conv_counts) {
  __shared__ int scan[256];
  __shared__ int hist[GMAXP];                  // choice 0..K-2 = candidate, K-1 = none
  const int rel = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
  const int role = P.role[rel];
  if (role == CSG_CANON_ROLE_PADDING || role == CSG_CANON_ROLE_IN_IMAGE) return;
  if (w.tot[((int64_t)b * P.P + rel) * 2] == 0) return;
  const int n = gen_n(w, P, b), nw = (n + 63) >> 6, K = P.K, q = P.rank[rel];
  if (tid < K) hist[tid] = 0;
  const uint64_t* U = w.U + (((int64_t)b * P.P + rel) * MAXN) * W;
  int c = 0;
  if (tid < n)
    for (int k = 0; k < nw; ++k) c += __popcll(U[tid * W + k]);
  int total = 0;
  int64_t k0 = u_off[b] + w.doff[(int64_t)b * P.P + rel] + block_exscan(c, scan, &total);   // syncs: hist is zero
  const double* cd = cdf + (int64_t)rel * K;
  if (tid < n) {
    const int s = tid;
    for (int k = 0; k < nw; ++k) {
      uint64_t m = U[s * W + k];
      while (m) {
        const int o = k * 64 + pop_bit(m);
        const int lo = choice_right(cd, K, uniforms[k0++]);
        atomicAdd(&hist[lo], 1);
        if (lo < K - 1) {                                      // converse edge (o, cand, s)
          const int cand = P.nm[lo + (lo >= q)];
          atomicOr((unsigned long long*)&w.V[(((int64_t)b * P.P + cand) * MAXN + o) * W + (s >> 6)], 1ull << (s & 63));
          w.flag[(int64_t)b * P.P + cand] = 1;
        }
      }
    }
  }
  __syncthreads();
  if (tid < K) {                                               // conv_counts[b][rel][r] (base_dataset.py:93), r = P: none
    const int col = tid < K - 1 ? P.nm[tid + (tid >= q)] : P.P;
    conv_counts[((int64_t)b * P.P + rel) * (P.P + 1) + col] = (float)hist[tid];
  }
}

// ---- close (base_dataset.py:109-120, graphs_utils.py:15-27,96-100): block (p, b)
__global__ __launch_bounds__(256) void k_gen_close(GenParams P, GenWs w) {
  __shared__ uint64_t adj[MAXN][W];
  __shared__ int scan[256];
  const int p = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
  const int64_t bp = (int64_t)b * P.P + p;
  const int conv = w.flag[bp];
  if (w.tot[bp * 2] == 0 && !conv) return;                     // empty predicate: tot stays {0, 0}
  const int role = P.role[p];
  const bool meta = role == CSG_CANON_ROLE_PADDING || role == CSG_CANON_ROLE_IN_IMAGE;
  const int n = gen_n(w, P, b), nw = (n + 63) >> 6;
  uint64_t* U = w.U + bp * MAXN * W;
  uint64_t* V = w.V + bp * MAXN * W;
  uint64_t cur[W] = {0, 0, 0, 0};             // the current graph's row, kept for closure - current
  int c = 0;
  if (tid < n) {
#pragma unroll
    for (int k = 0; k < W; ++k) {
      if (k < nw) {
        cur[k] = U[tid * W + k] | V[tid * W + k];
        if (conv) U[tid * W + k] = cur[k];
        adj[tid][k] = cur[k];
        c += __popcll(cur[k]);
      }
    }
    w.rc[bp * MAXN + tid] = c;
  }
  const int n_orig = block_sum(c, scan);
  int n_x = 0;
  if (P.learned_transitivity && !meta) {
    for (int i = 0; i < n; ++i) {
      __syncthreads();
      uint64_t any = 0;
      for (int k = 0; k < nw; ++k) any |= adj[i][k];
      if (!any) continue;                                      // an empty row i adds nothing (uniform: LDS read after a barrier)
      if (tid < n && tid != i && ((adj[tid][i >> 6] >> (i & 63)) & 1ull))
        for (int k = 0; k < nw; ++k) adj[tid][k] |= adj[i][k];
    }
    __syncthreads();
    int cx = 0;
    if (tid < n) {
#pragma unroll
      for (int k = 0; k < W; ++k) {
        if (k < nw) {
          const uint64_t x = adj[tid][k] & ~cur[k];
          V[tid * W + k] = x;
          cx += __popcll(x);
        }
      }
      w.xc[bp * MAXN + tid] = cx;
    }
    n_x = block_sum(cx, scan);
  }
  if (tid == 0) {
    w.tot[bp * 2 + 0] = n_orig;
    w.tot[bp * 2 + 1] = n_x;
  }
}

// ---- offsets: block b, thread s.  rc / xc become output positions in place.
__global__ __launch_bounds__(256) void k_gen_offsets(GenParams P, GenWs w, int64_t* __restrict__ counts) {
  __shared__ int scan[256];
  __shared__ int tot[GMAXP][2];
  const int b = blockIdx.x, tid = threadIdx.x;
  const int n = gen_n(w, P, b);
  if (tid < P.P) {
    tot[tid][0] = w.tot[((int64_t)b * P.P + tid) * 2 + 0];
    tot[tid][1] = w.tot[((int64_t)b * P.P + tid) * 2 + 1];
  }
  __syncthreads();
  int c = 0;
  if (tid < n)
    for (int p = 0; p < P.P; ++p)
      if (tot[p][0]) c += w.rc[((int64_t)b * P.P + p) * MAXN + tid];
  int n_orig = 0;
  int at = block_exscan(c, scan, &n_orig);                     // (s, p, o): rows first, predicates by ascending id
  if (tid < n)
    for (int p = 0; p < P.P; ++p) {
      if (!tot[p][0]) continue;
      int* rc = w.rc + ((int64_t)b * P.P + p) * MAXN + tid;
      const int v = *rc;
      *rc = at;
      at += v;
    }
  int run = n_orig;                                            // (p, s, o): the extras after every original
  for (int p = 0; p < P.P; ++p) {
    if (!tot[p][1]) continue;                                  // uniform: tot is in LDS
    int* xc = w.xc + ((int64_t)b * P.P + p) * MAXN + tid;
    const int v = tid < n ? *xc : 0;
    int t = 0;
    const int e = block_exscan(v, scan, &t);
    if (tid < n) *xc = run + e;
    run += t;
  }
  if (tid == 0) {
    counts[b * 2 + 0] = w.bad[b] ? -1 - (int64_t)n_orig : n_orig;    // negative: a device row was refused
    counts[b * 2 + 1] = run - n_orig;
  }
}

// ---- emit: block (p, b) writes the originals and the extras of predicate p, and a share of the padding
__global__ __launch_bounds__(256) void k_gen_emit(GenParams P, GenWs w, const int64_t* __restrict__ counts, int64_t T,
                                                  int64_t* __restrict__ triplets, int64_t* __restrict__ ttype) {
  const int p = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
  const int64_t bp = (int64_t)b * P.P + p;
  int64_t* trip = triplets + (int64_t)b * T * 3;
  int64_t* tt = ttype + (int64_t)b * T;
  const int n = gen_n(w, P, b), nw = (n + 63) >> 6;
  const int n_orig = w.tot[bp * 2 + 0], n_x = w.tot[bp * 2 + 1];
  if (tid < n && n_orig) {
    int64_t at = w.rc[bp * MAXN + tid];
    const uint64_t* U = w.U + (bp * MAXN + tid) * W;
    for (int k = 0; k < nw; ++k) at = emit_bits(U[k], k * 64, at, T, trip, tt, tid, p, 0);
  }
  if (tid < n && n_x) {
    int64_t at = w.xc[bp * MAXN + tid];
    const uint64_t* X = w.V + (bp * MAXN + tid) * W;
    for (int k = 0; k < nw; ++k) at = emit_bits(X[k], k * 64, at, T, trip, tt, tid, p, 1);
  }
  const int64_t used = counts[b * 2 + 0] + counts[b * 2 + 1];
  for (int64_t t = used + (int64_t)p * 256 + tid; t < T; t += (int64_t)P.P * 256)    // vg_collate_fn: packed_vg.py:207-212
    put_triplet(trip, tt, t, T, 0, P.pid_padding, 0, 0);
}

// ---- pack: annotated rows that are already on the device -> the workspace's 4-byte form (csg_canon_general_build_dev).
// One thread per (sample, row); rbeg came from the host's counts.  The host cannot check these rows, so nothing is indexed
// with one: a row outside [0, n_b) x [0, P), or carrying __padding__, is stored as a predicate no block owns (0xFFFF) and
// marks its sample in `bad`; k_gen_draws / k_gen_offsets then report a negative count.  Every thread that stores to bad[b]
// stores the same 1.
constexpr uint32_t kDroppedRow = 0xFFFF0000u;

__global__ __launch_bounds__(256) void k_gen_pack(GenParams P, GenWs w, const int64_t* __restrict__ rel, int R) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= (int64_t)P.B * R) return;
  const int b = (int)(i / R), r = (int)(i - (int64_t)b * R);
  const int r0 = w.rbeg[b];
  if (r >= w.rbeg[b + 1] - r0) return;
  const int n = gen_n(w, P, b);
  const int64_t s = rel[i * 3 + 0], p = rel[i * 3 + 1], o = rel[i * 3 + 2];
  const bool ok = s >= 0 && s < n && o >= 0 && o < n && p >= 0 && p < P.P && p != P.pid_padding;
  w.rows[r0 + r] = ok ? ((uint32_t)s | (uint32_t)o << 8 | (uint32_t)p << 16) : kDroppedRow;
  if (!ok) w.bad[b] = 1;
}

// ---- sampled pairs (reference sg2im/data/coco.py:372-421): one predicate per (sample, object) from the pair the host drew.
// One thread per (sample, object) row `cur`: (s, o) = (cur, other), or (other, cur) when flipped; surrounding / inside by the
// reference's strict comparisons of x0, y0 and of x0 + w / 2, y0 + h / 2 (the box CENTRE: what the reference compares),
// otherwise the quadrant of atan2(dy, dx) of d = centers[s] - centers[o].  The reference takes math.atan2 in double of the
// fp32 differences and compares with multiples of pi / 4; the sector is decided here by exact comparisons of |dx|, |dy| and
// the signs instead, which agree with those four inequalities for every fp32 pair, ties and signed zeros included
// (tests/test_pair_cases.py): a device atan2 one ulp from glibc's would flip a predicate on a tie.
// fp32 in the reference's order, no contraction.  A row at or beyond counts[b], or whose `other` is not another counted
// row of its sample (the host refused that from its copies; a stale device buffer can still disagree), is the collate's
// padding [0, __padding__, 0]: nothing is indexed with it.
struct PairIds {
  int padding, below, above, left, right, inside, surrounding;
};

__global__ __launch_bounds__(256) void k_pair_relations(const float4* __restrict__ boxes, const float2* __restrict__ centers,
                                                        const int64_t* __restrict__ counts, const int32_t* __restrict__ other,
                                                        const uint8_t* __restrict__ flip, PairIds id, int use_converse, int B,
                                                        int O, int64_t* __restrict__ rows) {
#pragma clang fp contract(off)
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= B * O) return;
  const int b = i / O, cur = i - b * O;
  int64_t n = counts[b];
  n = n > O ? O : n;
  const int oth = other[i];
  int64_t rs = 0, rp = id.padding, ro = 0;
  if (cur < n && oth >= 0 && oth < n && oth != cur) {
    int s = cur, o = oth;
    if (flip[i]) {
      s = oth;
      o = cur;
    }
    const float4 sb = boxes[(int64_t)b * O + s], ob = boxes[(int64_t)b * O + o];
    const float2 cs = centers[(int64_t)b * O + s], co = centers[(int64_t)b * O + o];
    const float sx0 = sb.x, sy0 = sb.y, sx1 = sb.x + sb.z / 2.0f, sy1 = sb.y + sb.w / 2.0f;
    const float ox0 = ob.x, oy0 = ob.y, ox1 = ob.x + ob.z / 2.0f, oy1 = ob.y + ob.w / 2.0f;
    const float dx = cs.x - co.x, dy = cs.y - co.y;
    const float ax = fabsf(dx), ay = fabsf(dy);
    const bool neg = signbit(dx);
    int p;
    bool swap = false;
    if (sx0 < ox0 && sx1 > ox1 && sy0 < oy0 && sy1 > oy1) {
      p = id.surrounding;
    } else if (sx0 > ox0 && sx1 < ox1 && sy0 > oy0 && sy1 < oy1) {
      p = use_converse ? id.surrounding : id.inside;
      swap = use_converse;
    } else if (neg && ay <= ax) {
      p = id.left;
    } else if (!neg && (ay < ax || (ay == ax && dy <= 0.0f))) {
      p = use_converse ? id.left : id.right;
      swap = use_converse;
    } else if (dy < 0.0f) {
      p = id.above;
    } else {
      p = use_converse ? id.above : id.below;
      swap = use_converse;
    }
    rs = swap ? o : s;
    rp = p;
    ro = swap ? s : o;
  }
  rows[(int64_t)i * 3 + 0] = rs;
  rows[(int64_t)i * 3 + 1] = rp;
  rows[(int64_t)i * 3 + 2] = ro;
}

// roles -> GenParams and the eight ids of k_canon_build; 0 if the table is not a vocabulary's
int gen_params(GenParams* G, int32_t* pred_ids, const int32_t* roles, int64_t B, int64_t P, int64_t O, int64_t image_id,
               int include_dummies, int learned_transitivity) {
  int seen[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  G->B = (int)B;
  G->P = (int)P;
  G->O = (int)O;
  G->image_id = (int)image_id;
  G->include_dummies = include_dummies;
  G->learned_transitivity = learned_transitivity;
  G->K = 0;
  for (int p = 0; p < P; ++p) {
    const int r = roles[p];
    int slot;
    if (r == CSG_CANON_ROLE_PADDING) slot = 0;
    else if (r == CSG_CANON_ROLE_IN_IMAGE) slot = 1;
    else if (r >= 0 && r < NREL) slot = 2 + r;
    else if (r == CSG_CANON_ROLE_OTHER) slot = -1;
    else return 0;
    G->role[p] = (signed char)r;
    if (slot >= 0) {
      if (seen[slot]++) return 0;
      pred_ids[slot] = p;
    }
    if (slot != 0 && slot != 1) {
      G->rank[p] = (unsigned char)G->K;
      G->nm[G->K++] = (unsigned char)p;
    }
  }
  for (int k = 0; k < 8; ++k)
    if (!seen[k]) return 0;
  G->pid_padding = pred_ids[0];
  G->pid_in_image = pred_ids[1];
  return 1;
}

#define GEN_CHECK_COMMON(fn)                                                                                           \
  CSG_REQUIRE(B > 0 && P > 0, CSG_E_BADSHAPE, fn ": bad shape B=%ld P=%ld", (long)B, (long)P);                         \
  CSG_REQUIRE(P <= GMAXP, CSG_E_UNSUPPORTED, fn ": at most %d predicates (got %ld)", GMAXP, (long)P);                  \
  CSG_REQUIRE(roles && workspace, CSG_E_BADSHAPE, fn ": null argument");                                              \
  CSG_REQUIRE(workspace_bytes >= gen_layout(B, P, 0, nullptr, nullptr), CSG_E_BADSHAPE,                               \
              fn ": workspace too small (%ld bytes)", (long)workspace_bytes)

// What csg_canon_general_build and csg_canon_general_build_dev (`fn`) do alike, after GEN_CHECK_COMMON: the shapes, the
// role table, and the head of the upload, which lies in `up` as in the workspace: bad[B] = 0 | nob[B] = n_objs |
// rbeg[B + 1] = the first row of each sample when sample b has rel_counts[b] rows (R without rel_counts) | room for
// B * row_room packed rows.
struct GenUpload {
  GenParams G;
  int32_t ids[8];
  std::vector<char> up;
  int64_t head;                  // bytes before the rows
  int64_t* nob;
  int* rbeg;
};

int gen_build_prologue(const char* fn, bool no_null, const int64_t* n_objs, int64_t B, int64_t O, const int64_t* rel_counts,
                       int64_t R, int64_t row_room, const int32_t* roles, int64_t P, int64_t image_id, int include_dummies,
                       int64_t workspace_bytes, GenUpload* u) {
  CSG_REQUIRE(O > 0 && R >= 0 && B * R < (1ll << 31), CSG_E_BADSHAPE, "%s: bad shape O=%ld R=%ld", fn, (long)O, (long)R);
  CSG_REQUIRE(O <= MAXN, CSG_E_UNSUPPORTED, "%s: at most %d objects per sample (got %ld)", fn, MAXN, (long)O);
  CSG_REQUIRE(no_null, CSG_E_BADSHAPE, "%s: null argument", fn);
  CSG_REQUIRE(workspace_bytes >= gen_layout(B, P, R, nullptr, nullptr), CSG_E_BADSHAPE,
              "%s: workspace too small (%ld bytes, need %ld)", fn, (long)workspace_bytes,
              (long)gen_layout(B, P, R, nullptr, nullptr));
  CSG_REQUIRE(gen_params(&u->G, u->ids, roles, B, P, O, image_id, include_dummies, 0), CSG_E_BADSHAPE,
              "%s: the role table needs one __padding__, one __in_image__ and each location relation exactly once", fn);
  u->head = gen_align(B * 4) + gen_align(B * 8) + gen_align((B + 1) * 4);
  u->up.assign((size_t)(u->head + B * row_room * 4), 0);
  u->nob = (int64_t*)(u->up.data() + gen_align(B * 4));
  u->rbeg = (int*)(u->up.data() + gen_align(B * 4) + gen_align(B * 8));
  int nr = 0;
  for (int64_t b = 0; b < B; ++b) {
    const int64_t n = n_objs[b];
    CSG_REQUIRE(n >= 0 && n <= O, CSG_E_BADSHAPE, "%s: n_objs[%ld] = %ld outside [0, %ld]", fn, (long)b, (long)n, (long)O);
    const int64_t cnt = rel_counts ? rel_counts[b] : R;
    CSG_REQUIRE(cnt >= 0 && cnt <= R, CSG_E_BADSHAPE, "%s: rel_counts[%ld] = %ld outside [0, %ld]", fn, (long)b, (long)cnt,
                (long)R);
    u->nob[b] = n;
    u->rbeg[b] = nr;
    nr += (int)cnt;
  }
  u->rbeg[B] = nr;
  return CSG_OK;
}
}  // namespace

extern "C" {

int64_t csg_canon_workspace(int64_t B) { return B > 0 ? B * kWsBytesPerSample : -1; }

int csg_canon_build(const int64_t* objs0, const float* boxes, const float* centers, const int64_t* n_objs,
                    int64_t B, int64_t O, const int32_t* pred_ids, int64_t image_id, int include_dummies,
                    int learned_transitivity, void* workspace, int64_t workspace_bytes, int64_t* counts,
                    void* stream) {
  CSG_REQUIRE(B > 0 && O > 0, CSG_E_BADSHAPE, "csg_canon_build: bad shape B=%ld O=%ld", (long)B, (long)O);
  CSG_REQUIRE(O <= MAXN, CSG_E_UNSUPPORTED, "csg_canon_build: at most %d objects per sample (got %ld)", MAXN, (long)O);
  CSG_REQUIRE(workspace && workspace_bytes >= B * kWsBytesPerSample, CSG_E_BADSHAPE,
              "csg_canon_build: workspace too small (%ld bytes, need %ld)", (long)workspace_bytes,
              (long)(B * kWsBytesPerSample));
  CanonParams P;
  CSG_REQUIRE(fill_params(&P, O, pred_ids, image_id, include_dummies, learned_transitivity), CSG_E_BADSHAPE,
              "csg_canon_build: the eight predicate ids must be distinct");
  hipStream_t s = (hipStream_t)stream;
  ProfScope p(K_CANON_BUILD, (double)B * O * O, s);
  CSG_LAUNCH(k_canon_build, dim3((unsigned)B), dim3(256), 0, s, P, objs0, boxes, centers, n_objs, workspace,
                     counts);
  return check_launch("csg_canon_build");
}

int csg_canon_emit(const int64_t* objs0, const int64_t* n_objs, int64_t B, int64_t O, const int32_t* pred_ids,
                   int64_t image_id, int include_dummies, int learned_transitivity, const void* workspace,
                   const int64_t* counts, int64_t T, int64_t* triplets, int64_t* triplet_type, void* stream) {
  CSG_REQUIRE(B > 0 && O > 0 && O <= MAXN && T >= 0, CSG_E_BADSHAPE, "csg_canon_emit: bad shape B=%ld O=%ld T=%ld",
              (long)B, (long)O, (long)T);
  if (T == 0) return CSG_OK;
  CanonParams P;
  CSG_REQUIRE(fill_params(&P, O, pred_ids, image_id, include_dummies, learned_transitivity), CSG_E_BADSHAPE,
              "csg_canon_emit: the eight predicate ids must be distinct");
  hipStream_t s = (hipStream_t)stream;
  ProfScope p(K_CANON_EMIT, (double)B * T * 32, s);
  CSG_LAUNCH(k_canon_emit, dim3((unsigned)B), dim3(256), 0, s, P, objs0, n_objs, workspace, counts, T,
                     triplets, triplet_type);
  return check_launch("csg_canon_emit");
}

int csg_canon_converse(const int64_t* objs0, const int64_t* n_objs, int64_t B, int64_t O, const int32_t* pred_ids,
                       int64_t image_id, int include_dummies, int learned_transitivity, void* workspace,
                       const double* cdf, const double* uniforms, const int64_t* u_off, int64_t num_preds,
                       float* conv_counts, int64_t* counts, void* stream) {
  CSG_REQUIRE(B > 0 && O > 0 && O <= MAXN && num_preds >= 8, CSG_E_BADSHAPE, "csg_canon_converse: bad shape B=%ld O=%ld P=%ld",
              (long)B, (long)O, (long)num_preds);
  CSG_REQUIRE(workspace && cdf && uniforms && u_off && conv_counts && counts, CSG_E_BADSHAPE, "csg_canon_converse: null argument");
  CanonParams P;
  CSG_REQUIRE(fill_params(&P, O, pred_ids, image_id, include_dummies, learned_transitivity), CSG_E_BADSHAPE,
              "csg_canon_converse: the eight predicate ids must be distinct");
  for (int r = 0; r < NREL; ++r)
    CSG_REQUIRE(P.pid[r] >= 0 && P.pid[r] < num_preds, CSG_E_BADSHAPE, "csg_canon_converse: predicate id %d outside [0, %ld)",
                P.pid[r], (long)num_preds);
  hipStream_t s = (hipStream_t)stream;
  ProfScope p(K_CANON_BUILD, (double)B * O * O, s);
  CSG_LAUNCH(k_canon_converse, dim3((unsigned)B), dim3(256), 0, s, P, objs0, n_objs, workspace, cdf, uniforms, u_off,
             (int)num_preds, conv_counts, counts);
  return check_launch("csg_canon_converse");
}

int64_t csg_canon_general_workspace(int64_t B, int64_t P, int64_t R) {
  if (B <= 0 || P <= 0 || P > GMAXP || R < 0) return -1;
  return gen_layout(B, P, R, nullptr, nullptr);
}

int csg_canon_general_build(const int64_t* objs0, const float* boxes, const float* centers, const int64_t* n_objs,
                            int64_t B, int64_t O, const int64_t* rel, const int64_t* rel_counts, int64_t R,
                            const int32_t* roles, int64_t P, int64_t image_id, int include_dummies, void* workspace,
                            int64_t workspace_bytes, int64_t* counts, void* stream) {
  const char* fn = "csg_canon_general_build";
  GEN_CHECK_COMMON("csg_canon_general_build");
  GenUpload u;
  // every input is checked here, before anything is enqueued; `up` is zeros: `bad` stays 0
  int rc = gen_build_prologue(fn, objs0 && n_objs && counts && (R == 0 || rel) && (boxes != nullptr) == (centers != nullptr),
                              n_objs, B, O, rel_counts, R, R, roles, P, image_id, include_dummies, workspace_bytes, &u);
  if (rc != CSG_OK) return rc;
  const bool geometry = boxes != nullptr;      // boxes = centers = NULL: the location relations are the given rows alone
  uint32_t* rows = (uint32_t*)(u.up.data() + u.head);
  int nr = 0;
  for (int64_t b = 0; b < B; ++b) {            // the rows are packed sample after sample, the skipped ones left out
    const int64_t cnt = rel_counts ? rel_counts[b] : R;
    u.rbeg[b] = nr;
    for (int64_t r = 0; r < cnt; ++r) {
      const int64_t* t = rel + (b * R + r) * 3;
      rc = check_host_row(fn, !rel_counts, " or __padding__", t, b, r, P, u.G.pid_padding, u.nob[b]);
      if (rc < 0) return rc;
      if (rc) rows[nr++] = (uint32_t)t[0] | (uint32_t)t[2] << 8 | (uint32_t)t[1] << 16;
    }
  }
  u.rbeg[B] = nr;
  GenWs w;
  gen_layout(B, P, R, workspace, &w);
  hipStream_t st = (hipStream_t)stream;
  // bad, nob, rbeg and rows are adjacent in the workspace, as in `up`; a pageable source is copied before the call returns
  CSG_REQUIRE(hipMemcpyAsync(w.bad, u.up.data(), (size_t)(u.head + (int64_t)nr * 4), hipMemcpyHostToDevice, st) == hipSuccess,
              CSG_E_LAUNCH, "csg_canon_general_build: upload of the annotated rows failed");
  CanonParams C;
  fill_params(&C, O, u.ids, image_id, 0, 0);
  if (geometry) {
    ProfScope pr(K_CANON_BUILD, (double)B * O * O, st);
    CSG_LAUNCH(k_canon_build, dim3((unsigned)B), dim3(256), 0, st, C, objs0, boxes, centers, (const int64_t*)w.nob,
               workspace, w.geo_counts);
  }
  {
    ProfScope pr(K_CANON_BUILD, (double)B * P * O * W, st);
    CSG_LAUNCH(k_gen_scatter, dim3((unsigned)P, (unsigned)B), dim3(256), 0, st, u.G, objs0, w,
               geometry ? workspace : (void*)nullptr);
    CSG_LAUNCH(k_gen_draws, dim3((unsigned)B), dim3(256), 0, st, u.G, w, counts);
  }
  return check_launch("csg_canon_general_build");
}

int csg_canon_general_converse(int64_t B, const int32_t* roles, int64_t P, void* workspace, int64_t workspace_bytes,
                               const double* cdf, const double* uniforms, const int64_t* u_off, float* conv_counts,
                               void* stream) {
  GEN_CHECK_COMMON("csg_canon_general_converse");
  CSG_REQUIRE(cdf && uniforms && u_off && conv_counts, CSG_E_BADSHAPE, "csg_canon_general_converse: null argument");
  GenParams G;
  int32_t ids[8];
  CSG_REQUIRE(gen_params(&G, ids, roles, B, P, 1, 0, 0, 0) && G.K >= 1, CSG_E_BADSHAPE,
              "csg_canon_general_converse: bad role table");
  GenWs w;
  gen_layout(B, P, 0, workspace, &w);
  hipStream_t st = (hipStream_t)stream;
  ProfScope pr(K_CANON_BUILD, (double)B * P * MAXN, st);
  CSG_LAUNCH(k_gen_converse, dim3((unsigned)P, (unsigned)B), dim3(256), 0, st, G, w, cdf, uniforms, u_off, conv_counts);
  return check_launch("csg_canon_general_converse");
}

int csg_canon_general_close(int64_t B, const int32_t* roles, int64_t P, int learned_transitivity, void* workspace,
                            int64_t workspace_bytes, int64_t* counts, void* stream) {
  GEN_CHECK_COMMON("csg_canon_general_close");
  CSG_REQUIRE(counts, CSG_E_BADSHAPE, "csg_canon_general_close: null argument");
  GenParams G;
  int32_t ids[8];
  CSG_REQUIRE(gen_params(&G, ids, roles, B, P, 1, 0, 0, learned_transitivity), CSG_E_BADSHAPE,
              "csg_canon_general_close: bad role table");
  GenWs w;
  gen_layout(B, P, 0, workspace, &w);
  hipStream_t st = (hipStream_t)stream;
  ProfScope pr(K_CANON_BUILD, (double)B * P * MAXN * MAXN, st);
  CSG_LAUNCH(k_gen_close, dim3((unsigned)P, (unsigned)B), dim3(256), 0, st, G, w);
  CSG_LAUNCH(k_gen_offsets, dim3((unsigned)B), dim3(256), 0, st, G, w, counts);
  return check_launch("csg_canon_general_close");
}

int csg_canon_general_emit(int64_t B, const int32_t* roles, int64_t P, const void* workspace, int64_t workspace_bytes,
                           const int64_t* counts, int64_t T, int64_t* triplets, int64_t* triplet_type, void* stream) {
  GEN_CHECK_COMMON("csg_canon_general_emit");
  CSG_REQUIRE(T >= 0 && counts, CSG_E_BADSHAPE, "csg_canon_general_emit: bad shape T=%ld", (long)T);
  if (T == 0) return CSG_OK;
  CSG_REQUIRE(triplets && triplet_type, CSG_E_BADSHAPE, "csg_canon_general_emit: null argument");
  GenParams G;
  int32_t ids[8];
  CSG_REQUIRE(gen_params(&G, ids, roles, B, P, 1, 0, 0, 0), CSG_E_BADSHAPE, "csg_canon_general_emit: bad role table");
  GenWs w;
  gen_layout(B, P, 0, (void*)workspace, &w);
  hipStream_t st = (hipStream_t)stream;
  ProfScope pr(K_CANON_EMIT, (double)B * T * 32, st);
  CSG_LAUNCH(k_gen_emit, dim3((unsigned)P, (unsigned)B), dim3(256), 0, st, G, w, counts, T, triplets, triplet_type);
  return check_launch("csg_canon_general_emit");
}

int csg_canon_general_build_dev(const int64_t* objs0, const float* boxes, const float* centers, const int64_t* n_objs,
                                int64_t B, int64_t O, const int64_t* rel, const int64_t* rel_counts, int64_t R,
                                const int32_t* roles, int64_t P, int64_t image_id, int include_dummies, void* workspace,
                                int64_t workspace_bytes, int64_t* counts, void* stream) {
  const char* fn = "csg_canon_general_build_dev";
  GEN_CHECK_COMMON("csg_canon_general_build_dev");
  CSG_REQUIRE(boxes == nullptr && centers == nullptr, CSG_E_UNSUPPORTED,
              "csg_canon_general_build_dev: boxes and centers must be NULL (the given rows are the whole graph)");
  CSG_REQUIRE(((uintptr_t)rel & 7) == 0, CSG_E_BADSHAPE, "csg_canon_general_build_dev: rel must be 8-byte aligned");
  GenUpload u;
  // what the host has is checked here, before anything is enqueued; the rows themselves by k_gen_pack
  const int rc = gen_build_prologue(fn, objs0 && n_objs && counts && rel_counts && (R == 0 || rel), n_objs, B, O, rel_counts, R,
                                    0, roles, P, image_id, include_dummies, workspace_bytes, &u);
  if (rc != CSG_OK) return rc;
  const int nr = u.rbeg[B];
  GenWs w;
  gen_layout(B, P, R, workspace, &w);
  hipStream_t st = (hipStream_t)stream;
  CSG_REQUIRE(hipMemcpyAsync(w.bad, u.up.data(), (size_t)u.head, hipMemcpyHostToDevice, st) == hipSuccess, CSG_E_LAUNCH,
              "csg_canon_general_build_dev: upload of the row offsets failed");
  {
    ProfScope pr(K_CANON_BUILD, (double)B * P * O * W, st);
    if (nr > 0) CSG_LAUNCH(k_gen_pack, dim3((unsigned)cdiv(B * R, 256)), dim3(256), 0, st, u.G, w, rel, (int)R);
    CSG_LAUNCH(k_gen_scatter, dim3((unsigned)P, (unsigned)B), dim3(256), 0, st, u.G, objs0, w, (void*)nullptr);
    CSG_LAUNCH(k_gen_draws, dim3((unsigned)B), dim3(256), 0, st, u.G, w, counts);
  }
  return check_launch("csg_canon_general_build_dev");
}

int csg_pair_relations(const float* boxes, const float* centers, const int64_t* counts, const int32_t* other,
                       const uint8_t* flip, const int64_t* counts_host, const int32_t* other_host, const uint8_t* flip_host,
                       int64_t B, int64_t O, const int32_t* pred_ids, int use_converse, int64_t* rows, void* stream) {
  CSG_REQUIRE(B >= 1 && O >= 1 && B * O < (1ll << 31), CSG_E_BADSHAPE, "csg_pair_relations: bad shape B=%ld O=%ld", (long)B,
              (long)O);
  CSG_REQUIRE(O <= MAXN, CSG_E_UNSUPPORTED, "csg_pair_relations: at most %d objects per sample (got %ld)", MAXN, (long)O);
  CSG_REQUIRE(boxes && centers && counts && other && flip && counts_host && other_host && flip_host && pred_ids && rows,
              CSG_E_BADSHAPE, "csg_pair_relations: null operand");
  CSG_REQUIRE(((uintptr_t)boxes & 15) == 0 && (((uintptr_t)centers | (uintptr_t)counts | (uintptr_t)rows) & 7) == 0 &&
                  ((uintptr_t)other & 3) == 0,
              CSG_E_BADSHAPE,
              "csg_pair_relations: boxes must be 16-byte aligned, centers, counts and rows 8-byte aligned, other 4-byte aligned");
  for (int a = 0; a < 8; ++a) {
    CSG_REQUIRE(pred_ids[a] >= 0, CSG_E_BADSHAPE, "csg_pair_relations: predicate id %d is negative", (int)pred_ids[a]);
    for (int c = a + 1; c < 8; ++c)
      CSG_REQUIRE(pred_ids[a] != pred_ids[c], CSG_E_BADSHAPE, "csg_pair_relations: the eight predicate ids must be distinct");
  }
  for (int64_t b = 0; b < B; ++b) {
    const int64_t n = counts_host[b];
    CSG_REQUIRE(n >= 0 && n <= O, CSG_E_BADSHAPE, "csg_pair_relations: sample %ld has %ld rows, 0 .. O = %ld", (long)b, (long)n,
                (long)O);
    for (int64_t i = 0; i < n; ++i) {
      const int64_t j = other_host[b * O + i];
      CSG_REQUIRE(j >= 0 && j < n && j != i, CSG_E_BADSHAPE,
                  "csg_pair_relations: sample %ld row %ld: other = %ld, another row of [0, %ld)", (long)b, (long)i, (long)j,
                  (long)n);
      CSG_REQUIRE(flip_host[b * O + i] <= 1, CSG_E_BADSHAPE, "csg_pair_relations: sample %ld row %ld: flip = %d, 0 or 1",
                  (long)b, (long)i, (int)flip_host[b * O + i]);
    }
  }
  PairIds id;        // pred_ids: __padding__ __in_image__ __below__ __above__ __left of__ __right of__ __inside__ __surrounding__
  id.padding = pred_ids[0];
  id.below = pred_ids[2];
  id.above = pred_ids[3];
  id.left = pred_ids[4];
  id.right = pred_ids[5];
  id.inside = pred_ids[6];
  id.surrounding = pred_ids[7];
  hipStream_t s = (hipStream_t)stream;
  ProfScope p(K_CANON_BUILD, (double)B * O, s);
  CSG_LAUNCH(k_pair_relations, dim3((unsigned)cdiv(B * O, 256)), dim3(256), 0, s, (const float4*)boxes, (const float2*)centers,
             counts, other, flip, id, use_converse ? 1 : 0, (int)B, (int)O, rows);
  return check_launch("csg_pair_relations");
}

}  // extern "C"
