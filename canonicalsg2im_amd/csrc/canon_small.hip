// Canonical graphs of at most 64 rows per sample from annotated relationships alone, one block per sample in one launch
// (csg_canon_small_*).  The unpacked Visual Genome dataset (reference sg2im/data/vg.py:136-149): the annotated rows and the
// __in_image__ dummies go through add_learnt_triplets (sg2im/data/base_dataset.py:89-139) — no location relation, no
// geometry, no role table: every predicate but __padding__ and __in_image__ is an ordinary non-meta predicate.
//
// The result is what k_gen_scatter -> k_gen_draws -> k_gen_converse -> k_gen_close -> k_gen_offsets (canon.hip) leave for a
// graph without boxes, and the phases below keep their order.  What differs is the shape of the work: a graph of <= 64
// objects is ONE 64-bit word per row of a predicate, so a predicate's 64x64 bit matrix is one register per lane of a
// wave64.  A wave owns a predicate: popcounts and prefix sums are wave scans, and Warshall's closure reads row k with two
// v_readlane (k is the loop counter, so it is wave-uniform) — no LDS matrix and no barrier inside the closure.
//
// U / V (originals / converse edges, then extras) live in a global workspace of 1 KiB per (sample, predicate): P = 256
// would need 256 KiB of LDS, more than a CU has, and one path serves every P.  The kernel touches them four times per
// predicate (zero, scatter / converse atomicOr, one read into registers, one write of the result), a block's share at
// P = 47 is 47 KiB, and it stays in L2.  The words that other waves of the block set with atomicOr (which act in L2) are
// read back with agent-scope atomic loads after the barrier, never through a line the CU's L1 may still hold.
// Integer atomics (OR, and counting draws) only: the bytes do not depend on the order in which waves run.
#include "csg_bitgraph.h"

using namespace csg;

namespace {

constexpr int SMAXN = 64;        // rows per sample, the __image__ row included: one lane each
constexpr int SMAXP = 256;       // predicates of a vocabulary
constexpr int SNT = 512;         // threads per block
constexpr int SNW = SNT / 64;    // waves per block: a wave takes predicates wave, wave + SNW, ...

struct SmallParams {
  int B, P, O, R;
  int K;                         // non-meta predicates = P - 2; a draw chooses among K - 1 candidates and "none"
  int m0, m1;                    // the two meta predicate ids, m0 < m1
  int image_id;
  int pid_padding, pid_in_image;
  int include_dummies, learned_transitivity;
};

// workspace of a sample: U[P][64] | V[P][64] (u64) | offo[P][64] | offx[P][64] | tot[P][2] (i32)
__host__ __device__ inline int64_t small_align(int64_t x) { return (x + 255) & ~(int64_t)255; }
__host__ __device__ inline int64_t small_bytes(int64_t P) {
  return small_align(P * SMAXN * 8 * 2 + P * SMAXN * 4 * 2 + P * 2 * 4);
}
struct SmallWs {
  uint64_t *U, *V;
  int *offo, *offx, *tot;
};
__host__ __device__ inline SmallWs small_ws(void* base, int64_t P, int64_t b) {
  char* at = (char*)base + b * small_bytes(P);
  SmallWs w;
  w.U = (uint64_t*)at;
  w.V = w.U + P * SMAXN;
  w.offo = (int*)(w.V + P * SMAXN);
  w.offx = w.offo + P * SMAXN;
  w.tot = w.offx + P * SMAXN;
  return w;
}

__device__ __forceinline__ bool is_meta(const SmallParams& S, int p) { return p == S.m0 || p == S.m1; }
// position of a non-meta predicate among the non-meta ones by ascending id, and back
__device__ __forceinline__ int nm_rank(const SmallParams& S, int p) { return p - (p > S.m0) - (p > S.m1); }
__device__ __forceinline__ int nm_pred(const SmallParams& S, int j) {
  int p = j + (j >= S.m0);
  return p + (p >= S.m1);
}

__device__ __forceinline__ uint64_t load_l2(const uint64_t* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// exclusive scan of one int of each of the first 256 threads; every thread of the block calls it
__device__ int scan256(int v, int* sm, int* total) {
  const int tid = threadIdx.x;
  const bool in = tid < 256;
  __syncthreads();
  if (in) sm[tid] = v;
  __syncthreads();
  for (int o = 1; o < 256; o <<= 1) {
    const int t = (in && tid >= o) ? sm[tid - o] : 0;
    __syncthreads();
    if (in) sm[tid] += t;
    __syncthreads();
  }
  *total = sm[255];
  return in ? sm[tid] - v : 0;
}

__global__ __launch_bounds__(SNT) void k_canon_small_build(SmallParams S, const int64_t* __restrict__ objs0,
                                                           const int64_t* __restrict__ n_objs,
                                                           const int64_t* __restrict__ rel, void* __restrict__ ws,
                                                           const double* __restrict__ cdf,
                                                           const double* __restrict__ uniforms,
                                                           const int64_t* __restrict__ u_off, int64_t n_uniforms,
                                                           float* __restrict__ conv_counts, int64_t* __restrict__ counts) {
  __shared__ int scan[256];
  __shared__ int tot_o[SMAXP], tot_x[SMAXP], doff[SMAXP], flag[SMAXP];
  __shared__ int hist[SNW][SMAXP];                 // a wave's draws of one predicate: choice 0..K-2 = candidate, K-1 = none
  __shared__ unsigned char cnt_o[SMAXP][SMAXN], cnt_x[SMAXP][SMAXN];   // originals / extras per (predicate, row): <= 64
  __shared__ int bad, n_orig_s;
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int P = S.P, K = S.K;
  int n = (int)n_objs[b];
  n = n < 0 ? 0 : (n > SMAXN ? SMAXN : n);
  if (n > S.O) n = S.O;
  const SmallWs w = small_ws(ws, P, b);

  // ---- zero
  for (int i = tid; i < P * SMAXN; i += SNT) {
    w.U[i] = 0;
    w.V[i] = 0;
  }
  if (tid < SMAXP) tot_o[tid] = tot_x[tid] = doff[tid] = flag[tid] = 0;
  if (tid == 0) bad = 0;
  // the __image__ object's index (base_dataset.py:144): the first of the sample's rows that carries the id
  const uint64_t is_img = __ballot(lane < n && objs0[(int64_t)b * S.O + lane] == (int64_t)S.image_id);
  const int img = (S.include_dummies && is_img) ? __ffsll((long long)is_img) - 1 : -1;
  __syncthreads();

  // ---- scatter: U[p] = the annotated rows of p (np.unique: a bit is set once) | the __in_image__ dummies
  const int64_t* rows = rel + (int64_t)b * S.R * 3;
  for (int r = tid; r < S.R; r += SNT) {             // vg.py:136-146
    const int64_t s = rows[r * 3 + 0], p = rows[r * 3 + 1], o = rows[r * 3 + 2];
    if (p == S.pid_padding) continue;
    // the host refused such a row from its copy; a device buffer that disagrees is not indexed with
    if (p < 0 || p >= P || s < 0 || s >= n || o < 0 || o >= n) {
      bad = 1;
      continue;
    }
    atomicOr((unsigned long long*)&w.U[p * SMAXN + s], 1ull << o);
  }
  if (wave == 0 && img >= 0 && lane < n && lane != img)       // base_dataset.py:141-151
    atomicOr((unsigned long long*)&w.U[S.pid_in_image * SMAXN + lane], 1ull << img);
  __syncthreads();

  // ---- draws: rows per predicate; the first draw of each non-meta predicate's rows (predicates by ascending id)
  for (int p = wave; p < P; p += SNW) {
    const int inc = wave_incscan(__popcll(load_l2(&w.U[p * SMAXN + lane])), lane);
    if (lane == 63) tot_o[p] = inc;
  }
  __syncthreads();
  int draws = 0;
  {
    const int c = (tid < P && !is_meta(S, tid)) ? tot_o[tid] : 0;
    const int ex = scan256(c, scan, &draws);
    if (tid < P) doff[tid] = ex;
  }

  // ---- converse (base_dataset.py:104-107, graphs_utils.py:126-152): a wave draws for the rows of its predicate, one
  // uniform per row in (s, o) order; converse edges are OR-ed into V of the chosen predicate
  if (cdf != nullptr) {
    for (int p0 = 0; p0 < P; p0 += SNW) {              // the same trip count in every wave: barriers inside
      const int rel_p = p0 + wave;
      const bool act = rel_p < P && !is_meta(S, rel_p) && tot_o[rel_p] > 0;
      const int q = act ? nm_rank(S, rel_p) : 0;
      if (act)
        for (int j = lane; j < K; j += 64) hist[wave][j] = 0;
      __syncthreads();
      if (act) {
        uint64_t m = load_l2(&w.U[rel_p * SMAXN + lane]);
        const int c = __popcll(m);
        int64_t k = u_off[b] + doff[rel_p] + (wave_incscan(c, lane) - c);
        const double* cd = cdf + (int64_t)rel_p * K;
        while (m) {
          const int o = pop_bit(m);
          const int64_t at = k++;
          if (at < 0 || at >= n_uniforms) {            // fewer numbers than rows: the host counted other rows than these
            bad = 1;
            continue;
          }
          const double u = uniforms[at];
          const int lo = choice_right(cd, K, u);
          atomicAdd(&hist[wave][lo], 1);
          if (lo < K - 1) {                            // converse edge (o, cand, s)
            const int cand = nm_pred(S, lo + (lo >= q));
            atomicOr((unsigned long long*)&w.V[cand * SMAXN + o], 1ull << lane);
            flag[cand] = 1;
          }
        }
      }
      __syncthreads();
      if (act)                                         // conv_counts[b][rel][r] (base_dataset.py:93), r = P: none
        for (int j = lane; j < K; j += 64) {
          const int col = j < K - 1 ? nm_pred(S, j + (j >= q)) : P;
          conv_counts[((int64_t)b * P + rel_p) * (P + 1) + col] = (float)hist[wave][j];
        }
    }
  }
  __syncthreads();

  // ---- close (base_dataset.py:109-120, graphs_utils.py:15-27,96-100): U <- U | V, Warshall, V <- closure - U
  for (int p = wave; p < P; p += SNW) {
    const int conv = flag[p];
    if (tot_o[p] == 0 && !conv) continue;              // empty predicate: its totals stay 0
    const uint64_t cur = load_l2(&w.U[p * SMAXN + lane]) | load_l2(&w.V[p * SMAXN + lane]);
    if (conv) w.U[p * SMAXN + lane] = cur;
    const int c = __popcll(cur);
    cnt_o[p][lane] = (unsigned char)c;
    const int inc = wave_incscan(c, lane);
    if (lane == 63) tot_o[p] = inc;
    if (S.learned_transitivity && !is_meta(S, p)) {
      const uint64_t x = wave_close(cur, n, lane) & ~cur;
      w.V[p * SMAXN + lane] = x;
      const int cx = __popcll(x);
      cnt_x[p][lane] = (unsigned char)cx;
      const int incx = wave_incscan(cx, lane);
      if (lane == 63) tot_x[p] = incx;
    }
  }
  __syncthreads();

  // ---- offsets.  Originals in (s, p, o) order: rows first, predicates by ascending id
  if (wave == 0) {
    int c = 0;
    for (int p = 0; p < P; ++p)
      if (tot_o[p]) c += cnt_o[p][lane];
    const int inc = wave_incscan(c, lane);
    int at = inc - c;
    for (int p = 0; p < P; ++p) {
      if (!tot_o[p]) continue;
      w.offo[p * SMAXN + lane] = at;
      at += cnt_o[p][lane];
    }
    if (lane == 63) n_orig_s = inc;
  }
  int n_x = 0;                                         // extras in (p, s, o) order, after every original
  const int xbase = scan256(tid < P ? tot_x[tid] : 0, scan, &n_x);
  if (tid < P) doff[tid] = xbase;
  __syncthreads();
  const int n_orig = n_orig_s;
  for (int p = wave; p < P; p += SNW) {
    if (lane < 2) w.tot[p * 2 + lane] = lane ? tot_x[p] : tot_o[p];
    if (!tot_x[p]) continue;
    const int cx = cnt_x[p][lane];
    w.offx[p * SMAXN + lane] = n_orig + doff[p] + (wave_incscan(cx, lane) - cx);
  }
  if (tid == 0) {
    counts[b * 2 + 0] = bad ? -1 - (int64_t)n_orig : n_orig;        // negative: a device row was refused
    counts[b * 2 + 1] = n_x;
  }
}

// ---- emit: block b; a wave writes the originals and the extras of its predicates, every thread a share of the padding
__global__ __launch_bounds__(SNT) void k_canon_small_emit(int P, int pid_padding, const void* __restrict__ ws,
                                                          const int64_t* __restrict__ counts, int64_t T,
                                                          int64_t* __restrict__ triplets, int64_t* __restrict__ ttype) {
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const SmallWs w = small_ws((void*)ws, P, b);
  int64_t* trip = triplets + (int64_t)b * T * 3;
  int64_t* tt = ttype + (int64_t)b * T;
  for (int p = wave; p < P; p += SNW) {
    if (w.tot[p * 2 + 0]) emit_bits(w.U[p * SMAXN + lane], 0, w.offo[p * SMAXN + lane], T, trip, tt, lane, p, 0);
    if (w.tot[p * 2 + 1]) emit_bits(w.V[p * SMAXN + lane], 0, w.offx[p * SMAXN + lane], T, trip, tt, lane, p, 1);
  }
  int64_t used = counts[b * 2 + 0] + counts[b * 2 + 1];
  if (used < 0) used = 0;
  for (int64_t t = used + tid; t < T; t += SNT) put_triplet(trip, tt, t, T, 0, pid_padding, 0, 0);    // vg_collate_fn: vg.py:214-219
}

#define SMALL_CHECK_COMMON(fn)                                                                                          \
  CSG_REQUIRE(B > 0 && P > 0, CSG_E_BADSHAPE, fn ": bad shape B=%ld P=%ld", (long)B, (long)P);                          \
  CSG_REQUIRE(P <= SMAXP, CSG_E_UNSUPPORTED, fn ": at most %d predicates (got %ld)", SMAXP, (long)P);                   \
  CSG_REQUIRE(workspace, CSG_E_BADSHAPE, fn ": null argument");                                                        \
  CSG_REQUIRE(workspace_bytes >= B * small_bytes(P), CSG_E_BADSHAPE, fn ": workspace too small (%ld bytes, need %ld)", \
              (long)workspace_bytes, (long)(B * small_bytes(P)))

}  // namespace

extern "C" {

int64_t csg_canon_small_workspace(int64_t B, int64_t P) {
  if (B <= 0 || P <= 0 || P > SMAXP) return -1;
  return B * small_bytes(P);
}

int csg_canon_small_build(const int64_t* objs0, const int64_t* n_objs, const int64_t* n_objs_host, int64_t B, int64_t O,
                          const int64_t* rel, const int64_t* rel_host, int64_t R, int64_t P, int64_t pid_padding,
                          int64_t pid_in_image, int64_t image_id, int include_dummies, int learned_transitivity,
                          const double* cdf, const double* uniforms, const int64_t* u_off, int64_t n_uniforms,
                          float* conv_counts, void* workspace, int64_t workspace_bytes, int64_t* counts, void* stream) {
  SMALL_CHECK_COMMON("csg_canon_small_build");
  CSG_REQUIRE(O > 0 && O < (1ll << 31) && R >= 0 && R < (1ll << 31) / 3, CSG_E_BADSHAPE,
              "csg_canon_small_build: bad shape O=%ld R=%ld", (long)O, (long)R);
  CSG_REQUIRE(objs0 && n_objs && n_objs_host && counts && (R == 0 || (rel && rel_host)), CSG_E_BADSHAPE,
              "csg_canon_small_build: null argument");
  CSG_REQUIRE(((uintptr_t)rel & 7) == 0, CSG_E_BADSHAPE, "csg_canon_small_build: rel must be 8-byte aligned");
  if (const int rc = check_meta_ids("csg_canon_small_build", P, pid_padding, pid_in_image)) return rc;
  const bool converse = cdf != nullptr;
  CSG_REQUIRE(!converse || (uniforms && u_off && conv_counts && n_uniforms >= 0 && P >= 3), CSG_E_BADSHAPE,
              "csg_canon_small_build: the converse draws need uniforms, u_off, conv_counts and a non-meta predicate");
  // every input the host holds is checked here, before anything is enqueued
  for (int64_t b = 0; b < B; ++b) {
    const int64_t n = n_objs_host[b];
    CSG_REQUIRE(n >= 0 && n <= O, CSG_E_BADSHAPE, "csg_canon_small_build: n_objs[%ld] = %ld outside [0, %ld]", (long)b, (long)n,
                (long)O);
    CSG_REQUIRE(n <= SMAXN, CSG_E_UNSUPPORTED,
                "csg_canon_small_build: at most %d rows per sample, the __image__ row included (sample %ld has %ld)", SMAXN,
                (long)b, (long)n);
    for (int64_t r = 0; r < R; ++r) {
      const int rc = check_host_row("csg_canon_small_build", true, "", rel_host + (b * R + r) * 3, b, r, P, pid_padding, n);
      if (rc < 0) return rc;
    }
  }
  SmallParams S;
  S.B = (int)B;
  S.P = (int)P;
  S.O = (int)O;
  S.R = (int)R;
  S.K = (int)P - 2;
  S.m0 = (int)(pid_padding < pid_in_image ? pid_padding : pid_in_image);
  S.m1 = (int)(pid_padding < pid_in_image ? pid_in_image : pid_padding);
  S.image_id = (int)image_id;
  S.pid_padding = (int)pid_padding;
  S.pid_in_image = (int)pid_in_image;
  S.include_dummies = include_dummies ? 1 : 0;
  S.learned_transitivity = learned_transitivity ? 1 : 0;
  hipStream_t st = (hipStream_t)stream;
  ProfScope pr(K_CANON_SMALL_BUILD, (double)B * P * SMAXN, st);
  CSG_LAUNCH(k_canon_small_build, dim3((unsigned)B), dim3(SNT), 0, st, S, objs0, n_objs, rel, workspace, cdf, uniforms, u_off,
             n_uniforms, conv_counts, counts);
  return check_launch("csg_canon_small_build");
}

int csg_canon_small_emit(int64_t B, int64_t P, int64_t pid_padding, const void* workspace, int64_t workspace_bytes,
                         const int64_t* counts, int64_t T, int64_t* triplets, int64_t* triplet_type, void* stream) {
  SMALL_CHECK_COMMON("csg_canon_small_emit");
  CSG_REQUIRE(T >= 0 && counts && pid_padding >= 0 && pid_padding < P, CSG_E_BADSHAPE,
              "csg_canon_small_emit: bad shape T=%ld __padding__=%ld", (long)T, (long)pid_padding);
  if (T == 0) return CSG_OK;
  CSG_REQUIRE(triplets && triplet_type, CSG_E_BADSHAPE, "csg_canon_small_emit: null argument");
  hipStream_t st = (hipStream_t)stream;
  ProfScope pr(K_CANON_SMALL_EMIT, (double)B * T * 32, st);
  CSG_LAUNCH(k_canon_small_emit, dim3((unsigned)B), dim3(SNT), 0, st, (int)P, (int)pid_padding, workspace, counts, T, triplets,
             triplet_type);
  return check_launch("csg_canon_small_emit");
}

}  // extern "C"
