// The k-nearest-neighbour manifolds behind precision / recall and density / coverage (canonicalsg2im_amd/quality.py, DESIGN
// 4.19c).  As in quality.hip: no atomics, nothing read back, stream ordered, and every result the same bits on every run —
// the outputs are a k-th smallest value and integer counts, which do not depend on the order they are merged in; the merges
// still walk their partial results in index order.
//
//   k_knn_tiles / _fold    r2[i] = the k-th smallest d2(f_i, f_j), j != i: 64 x 64 tiles, each row keeps its k smallest
//   k_ball_tiles / _fold   inside[j] = #{i : d2(q_j, f_i) <= r2[i]}, holds[i] = #{j : the same}, both from one pass
//
// THE DISTANCE (man_d2_tile, the only one): d2(u, v) = sum_c t_c * t_c, t_c = (double)u_c - (double)v_c, columns in ascending
// order, each step ONE FUSED multiply-add acc = fma(t_c, t_c, acc) in fp64.  No |u|^2 + |v|^2 - 2 u.v: the difference form
// gives identical rows exactly 0, is symmetric bit for bit and exact on integer-valued features.  No n x m array exists in
// memory at any time.
#include <math.h>

#include "csg_common.h"

namespace csg {

constexpr int kManKD = 32;         // feature columns per stage, as k_kid_tiles: 2 x 32 x 68 floats = 17 KB of LDS
constexpr int kManLD = 68;         // 64 rows + 4: a stage row starts on a 16-byte boundary
constexpr int kManKMax = 16;       // the longest k-list
constexpr int kManListLD = 17;     // doubles per k-list: lane r's list starts 34 banks after lane r - 1's, 32 lanes on 64 banks
constexpr int kManTileLD = 65;     // entries per row of a tile handed through LDS: lane r reads row r, one bank step per lane
constexpr int64_t kManMaxRows = 1ll << 20;

// THE SPLIT RULE (csg_manifold_column_chunks).  `row_blocks` blocks stand side by side along the rows; the column tiles are
// cut into this many chunks, one more block each: at least two column tiles per chunk, at most 64 chunks, and no more than
// brings the launch to 8192 blocks (32 per CU: the last round of blocks is then a small share of the run).
static inline int64_t man_chunks(int64_t row_blocks, int64_t col_tiles) {
  int64_t c = cdiv(col_tiles, 2);
  c = c > 64 ? 64 : c;
  const int64_t fill = cdiv(8192, row_blocks);
  c = c > fill ? fill : c;
  return c < 1 ? 1 : c;
}

// acc[u][v] += d2(row a0 + ri * 4 + u of A, row b0 + rj * 4 + v of B) over all D columns, ri = thread / 16, rj = thread % 16.
// k_kid_tiles's staging: the two 64-row operands go KD columns at a time into LDS, transposed ([column][row]); a row past
// nA / nB is staged as zeros and never addressed.  Every thread of the block calls it; it begins with a barrier, so what the
// caller kept in the same LDS is dead by then, and the caller puts a barrier behind it before it reuses that LDS.
__device__ __forceinline__ void man_d2_tile(const float* __restrict__ A, int nA, int a0, const float* __restrict__ B, int nB,
                                            int b0, int D, float (*As)[kManLD], float (*Bs)[kManLD], double (&acc)[4][4]) {
  const int lr = threadIdx.x >> 3, q = threadIdx.x & 7;      // staging role: rows lr and lr + 32, the column quad q
  int64_t ra[2], rb[2];
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const int gi = a0 + lr + 32 * h, gj = b0 + lr + 32 * h;
    ra[h] = gi < nA ? (int64_t)gi * D + q * 4 : -1;
    rb[h] = gj < nB ? (int64_t)gj * D + q * 4 : -1;
  }
  const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
  float4 va[2], vb[2];
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    va[h] = ra[h] >= 0 ? *(const float4*)(A + ra[h]) : zero;
    vb[h] = rb[h] >= 0 ? *(const float4*)(B + rb[h]) : zero;
  }
  const int ri = threadIdx.x >> 4, rj = threadIdx.x & 15;
  for (int k0 = 0; k0 < D; k0 += kManKD) {
    __syncthreads();
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int row = lr + 32 * h;
      As[q * 4 + 0][row] = va[h].x, As[q * 4 + 1][row] = va[h].y, As[q * 4 + 2][row] = va[h].z, As[q * 4 + 3][row] = va[h].w;
      Bs[q * 4 + 0][row] = vb[h].x, Bs[q * 4 + 1][row] = vb[h].y, Bs[q * 4 + 2][row] = vb[h].z, Bs[q * 4 + 3][row] = vb[h].w;
    }
    __syncthreads();
    if (k0 + kManKD < D) {      // the next stage's rows travel while this one is worked on
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        va[h] = ra[h] >= 0 ? *(const float4*)(A + ra[h] + k0 + kManKD) : zero;
        vb[h] = rb[h] >= 0 ? *(const float4*)(B + rb[h] + k0 + kManKD) : zero;
      }
    }
#pragma unroll 8
    for (int d = 0; d < kManKD; ++d) {
      const float4 a = *(const float4*)&As[d][ri * 4];
      const float4 b = *(const float4*)&Bs[d][rj * 4];
      const double av[4] = {(double)a.x, (double)a.y, (double)a.z, (double)a.w};
      const double bv[4] = {(double)b.x, (double)b.y, (double)b.z, (double)b.w};
#pragma unroll
      for (int u = 0; u < 4; ++u) {
#pragma unroll
        for (int v = 0; v < 4; ++v) {
          const double t = av[u] - bv[v];
          acc[u][v] = fma(t, t, acc[u][v]);
        }
      }
    }
  }
}

// d < l[k - 1]: put d into the ascending list l[0 .. k), dropping its largest entry -> the new l[k - 1].  Equal values stay,
// as often as they came.
__device__ __forceinline__ double man_insert(double* l, int k, double d) {
  int j = k - 1;
  while (j > 0 && l[j - 1] > d) {
    l[j] = l[j - 1];
    --j;
  }
  l[j] = d;
  return l[k - 1];
}

// ------------------------------------------------------------------------------------------------ k-NN radii
// Block (ti, c): the rows of row tile ti against the column tiles of chunk c, [c T / chunks, (c + 1) T / chunks).  A finished
// tile goes through LDS (over the stages, which are dead by then) with +inf in the places that do not count: a column past
// n, and j = i — self is excluded by INDEX, a duplicate row at another index counts with its distance 0.  Lane r of wave 0
// owns row r's ascending k-list (LDS) and its k-th entry (a register) and inserts what is SMALLER than that entry; a NaN is
// smaller than nothing, so it ranks as +inf.  After a row's first tiles almost nothing passes.  The lists go to
// ws[c][row][k]; k_knn_fold merges a row's lists in chunk order the same way and keeps the k-th.
// Two things left as they are on purpose.  Only wave 0 inserts while the other three wait at the next barrier: a tile's
// scan is 64 LDS reads per lane against 32 D fp64 instructions per lane of tile work, under 1 % at D = 2048.  And the
// symmetry d2(i, j) = d2(j, i) is not used, every tile of the n x n matrix is computed: a tile mirrored into another block's
// rows would have to cross blocks through memory.  Measured 37 to 39 TFLOP/s (three operations per pair and column) where
// k_kid_tiles, which has neither cost, does 40.5 with two.
__global__ __launch_bounds__(256) void k_knn_tiles(const float* __restrict__ f, int n, int D, int k, int T, int chunks,
                                                   double* __restrict__ ws) {
  __shared__ __attribute__((aligned(16))) unsigned char raw[64 * kManTileLD * 8];      // 33 KB; the stages take 17 KB of it
  __shared__ double kl[64][kManListLD];
  float(*As)[kManLD] = (float(*)[kManLD])raw;
  float(*Bs)[kManLD] = As + kManKD;
  double(*dt)[kManTileLD] = (double(*)[kManTileLD])raw;
  const int ti = blockIdx.x, c = blockIdx.y;
  const int t0 = (int)((int64_t)c * T / chunks), t1 = (int)((int64_t)(c + 1) * T / chunks);
  const int ri = threadIdx.x >> 4, rj = threadIdx.x & 15;
  double kth = INFINITY;
  if (threadIdx.x < 64) {
    for (int j = 0; j < kManKMax; ++j) kl[threadIdx.x][j] = INFINITY;      // read and written by this lane alone
  }
  for (int tj = t0; tj < t1; ++tj) {
    double acc[4][4] = {};
    man_d2_tile(f, n, ti * 64, f, n, tj * 64, D, As, Bs, acc);
    __syncthreads();
#pragma unroll
    for (int u = 0; u < 4; ++u) {
#pragma unroll
      for (int v = 0; v < 4; ++v) {
        const int gi = ti * 64 + ri * 4 + u, gj = tj * 64 + rj * 4 + v;
        dt[ri * 4 + u][rj * 4 + v] = (gj < n && gj != gi) ? acc[u][v] : (double)INFINITY;
      }
    }
    __syncthreads();
    if (threadIdx.x < 64) {
      for (int cc = 0; cc < 64; ++cc) {
        const double d = dt[threadIdx.x][cc];
        if (d < kth) kth = man_insert(kl[threadIdx.x], k, d);
      }
    }
  }
  const int gi = ti * 64 + (int)threadIdx.x;
  if (threadIdx.x < 64 && gi < n) {
    double* out = ws + ((int64_t)c * n + gi) * k;
    for (int j = 0; j < k; ++j) out[j] = kl[threadIdx.x][j];
  }
}

__global__ __launch_bounds__(64) void k_knn_fold(const double* __restrict__ ws, int n, int k, int chunks,
                                                 double* __restrict__ r2) {
  __shared__ double kl[64][kManListLD];
  const int gi = blockIdx.x * 64 + threadIdx.x;
  if (gi >= n) return;
  for (int j = 0; j < kManKMax; ++j) kl[threadIdx.x][j] = INFINITY;
  double kth = INFINITY;
  for (int c = 0; c < chunks; ++c) {
    const double* in = ws + ((int64_t)c * n + gi) * k;
    for (int j = 0; j < k; ++j) {
      const double d = in[j];
      if (!(d < kth)) break;                 // a chunk's list ascends: nothing behind this entry is smaller either
      kth = man_insert(kl[threadIdx.x], k, d);
    }
  }
  r2[gi] = kth;
}

// ------------------------------------------------------------------------------------------------ ball counts
// The query tiles are cut into Gq row groups and the centre tiles into Gc chunks; block (gq, gc) walks every tile of its
// group pair, row tile by row tile.  Pair (j, i) is INSIDE when d2(q_j, f_i) is finite and <= r2[i] (a NaN or +inf distance
// is inside nothing, a NaN radius holds nothing; a query on the sphere is inside).  A tile's 64 x 64 flags go through LDS
// (over the dead stages): lane r of wave 0 adds row r, lane c of wave 1 adds column c.  The block is the only writer of
// ws_inside[gc][its rows] and ws_holds[gq][its columns], so it accumulates there with plain loads and stores, a row or a
// column always in the hands of the same thread; its first visit stores.  k_count_fold adds the groups in index order.
__global__ __launch_bounds__(256) void k_ball_tiles(const float* __restrict__ q, int m, const float* __restrict__ f, int n, int D,
                                                    const double* __restrict__ r2, int Tq, int Tf, int Gq, int Gc,
                                                    int* ws_inside, int* ws_holds) {
  __shared__ __attribute__((aligned(16))) unsigned char raw[2 * kManKD * kManLD * 4];      // 17 KB: the stages, then 64 x 65 flags
  static_assert(64 * kManTileLD * 4 <= 2 * kManKD * kManLD * 4, "the flags fit over the stages");
  float(*As)[kManLD] = (float(*)[kManLD])raw;
  float(*Bs)[kManLD] = As + kManKD;
  int(*fl)[kManTileLD] = (int(*)[kManTileLD])raw;
  const int gq = blockIdx.x, gc = blockIdx.y;
  const int r0 = (int)((int64_t)gq * Tq / Gq), r1 = (int)((int64_t)(gq + 1) * Tq / Gq);
  const int c0 = (int)((int64_t)gc * Tf / Gc), c1 = (int)((int64_t)(gc + 1) * Tf / Gc);
  const int ri = threadIdx.x >> 4, rj = threadIdx.x & 15;
  const int t = threadIdx.x;
  for (int ti = r0; ti < r1; ++ti) {
    int row_count = 0;
    for (int tj = c0; tj < c1; ++tj) {
      double acc[4][4] = {};
      double rr[4];
#pragma unroll
      for (int v = 0; v < 4; ++v) {
        const int gj = tj * 64 + rj * 4 + v;
        rr[v] = gj < n ? r2[gj] : -1.0;
      }
      man_d2_tile(q, m, ti * 64, f, n, tj * 64, D, As, Bs, acc);
      __syncthreads();
#pragma unroll
      for (int u = 0; u < 4; ++u) {
#pragma unroll
        for (int v = 0; v < 4; ++v) {
          const int gi = ti * 64 + ri * 4 + u, gj = tj * 64 + rj * 4 + v;
          fl[ri * 4 + u][rj * 4 + v] = (gi < m && gj < n && acc[u][v] < (double)INFINITY && acc[u][v] <= rr[v]) ? 1 : 0;
        }
      }
      __syncthreads();
      if (t < 64) {
        int s = 0;
        for (int cc = 0; cc < 64; ++cc) s += fl[t][cc];
        row_count += s;
      } else if (t < 128) {
        const int cc = t - 64, gj = tj * 64 + cc;
        int s = 0;
        for (int r = 0; r < 64; ++r) s += fl[r][cc];
        if (gj < n) {
          int* p = ws_holds + (int64_t)gq * n + gj;
          *p = (ti == r0 ? 0 : *p) + s;
        }
      }
    }
    if (t < 64 && ti * 64 + t < m) ws_inside[(int64_t)gc * m + ti * 64 + t] = row_count;
  }
}

// out_a[i] = sum_g ws_a[g][i] (na entries, ga groups), then out_b likewise: groups in index order
__global__ __launch_bounds__(256) void k_count_fold(const int* __restrict__ ws_a, int na, int ga, int* __restrict__ out_a,
                                                    const int* __restrict__ ws_b, int nb, int gb, int* __restrict__ out_b) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < na) {
    int s = 0;
    for (int g = 0; g < ga; ++g) s += ws_a[(int64_t)g * na + i];
    out_a[i] = s;
  } else if (i < (int64_t)na + nb) {
    const int64_t j = i - na;
    int s = 0;
    for (int g = 0; g < gb; ++g) s += ws_b[(int64_t)g * nb + j];
    out_b[j] = s;
  }
}

// the row groups of csg_ball_counts: one per query tile, at most 64
static inline int64_t ball_row_groups(int64_t m) {
  const int64_t T = cdiv(m, 64);
  return T > 64 ? 64 : T;
}

}  // namespace csg

using namespace csg;

extern "C" {

int64_t csg_manifold_column_chunks(int64_t rows, int64_t cols) {
  if (rows < 1 || cols < 1 || rows > kManMaxRows || cols > kManMaxRows) return -1;
  return man_chunks(cdiv(rows, 64), cdiv(cols, 64));
}

int64_t csg_knn_radii_workspace_bytes(int64_t n, int64_t k) {
  if (k < 1 || k > kManKMax || n < k + 1 || n > kManMaxRows) return -1;
  return csg_manifold_column_chunks(n, n) * n * k * 8;
}

int csg_knn_radii(const float* f, int64_t n, int64_t D, int64_t k, void* workspace, int64_t workspace_bytes, double* r2,
                  void* stream) {
  CSG_REQUIRE(f != nullptr && workspace != nullptr && r2 != nullptr, CSG_E_BADSHAPE, "csg_knn_radii: null operand");
  CSG_REQUIRE(k >= 1 && k <= kManKMax, CSG_E_BADSHAPE, "csg_knn_radii: k=%ld (served: 1 .. 16)", (long)k);
  CSG_REQUIRE(n >= k + 1 && n <= kManMaxRows, CSG_E_BADSHAPE,
              "csg_knn_radii: n=%ld rows for k=%ld (a row needs k others: k <= n - 1; n <= 2^20)", (long)n, (long)k);
  CSG_REQUIRE(D > 0 && D % 64 == 0 && D <= 8192, CSG_E_BADSHAPE, "csg_knn_radii: D=%ld (a multiple of 64, at most 8192)", (long)D);
  CSG_REQUIRE((uintptr_t)f % 16 == 0 && ((uintptr_t)workspace | (uintptr_t)r2) % 8 == 0, CSG_E_BADSHAPE,
              "csg_knn_radii: features must be 16-byte aligned, workspace and r2 8-byte aligned");
  CSG_REQUIRE(workspace_bytes >= csg_knn_radii_workspace_bytes(n, k), CSG_E_WORKSPACE, "csg_knn_radii: needs %lld bytes of workspace",
              (long long)csg_knn_radii_workspace_bytes(n, k));
  hipStream_t s = (hipStream_t)stream;
  const int T = (int)cdiv(n, 64);
  const int chunks = (int)csg_manifold_column_chunks(n, n);
  ProfScope p(K_KNN_RADII, (double)T * T * 64 * 64 * D * 3, s);      // per pair and column: a subtraction, a product, a sum
  CSG_LAUNCH(k_knn_tiles, dim3((unsigned)T, (unsigned)chunks), dim3(256), 0, s, f, (int)n, (int)D, (int)k, T, chunks,
             (double*)workspace);
  CSG_LAUNCH(k_knn_fold, dim3((unsigned)T), dim3(64), 0, s, (const double*)workspace, (int)n, (int)k, chunks, r2);
  return check_launch("csg_knn_radii");
}

int64_t csg_ball_counts_workspace_bytes(int64_t m, int64_t n) {
  if (m < 1 || n < 1 || m > kManMaxRows || n > kManMaxRows) return -1;
  const int64_t Gq = ball_row_groups(m);
  return (m * man_chunks(Gq, cdiv(n, 64)) + n * Gq) * 4;
}

int csg_ball_counts(const float* q, int64_t m, const float* f, int64_t n, int64_t D, const double* r2, void* workspace,
                    int64_t workspace_bytes, int32_t* inside, int32_t* holds, void* stream) {
  CSG_REQUIRE(q != nullptr && f != nullptr && r2 != nullptr && workspace != nullptr && inside != nullptr && holds != nullptr,
              CSG_E_BADSHAPE, "csg_ball_counts: null operand");
  CSG_REQUIRE(m >= 1 && n >= 1 && m <= kManMaxRows && n <= kManMaxRows, CSG_E_BADSHAPE,
              "csg_ball_counts: m=%ld queries, n=%ld centres (1 .. 2^20 each)", (long)m, (long)n);
  CSG_REQUIRE(D > 0 && D % 64 == 0 && D <= 8192, CSG_E_BADSHAPE, "csg_ball_counts: D=%ld (a multiple of 64, at most 8192)", (long)D);
  CSG_REQUIRE(((uintptr_t)q | (uintptr_t)f) % 16 == 0 && (uintptr_t)r2 % 8 == 0 &&
                  ((uintptr_t)workspace | (uintptr_t)inside | (uintptr_t)holds) % 4 == 0,
              CSG_E_BADSHAPE, "csg_ball_counts: features must be 16-byte aligned, r2 8-byte, workspace and counts 4-byte aligned");
  CSG_REQUIRE(workspace_bytes >= csg_ball_counts_workspace_bytes(m, n), CSG_E_WORKSPACE,
              "csg_ball_counts: needs %lld bytes of workspace", (long long)csg_ball_counts_workspace_bytes(m, n));
  hipStream_t s = (hipStream_t)stream;
  const int Tq = (int)cdiv(m, 64), Tf = (int)cdiv(n, 64);
  const int Gq = (int)ball_row_groups(m), Gc = (int)man_chunks(Gq, Tf);
  int* ws_inside = (int*)workspace;
  int* ws_holds = ws_inside + m * Gc;
  ProfScope p(K_BALL_COUNTS, (double)Tq * Tf * 64 * 64 * D * 3, s);
  CSG_LAUNCH(k_ball_tiles, dim3((unsigned)Gq, (unsigned)Gc), dim3(256), 0, s, q, (int)m, f, (int)n, (int)D, r2, Tq, Tf, Gq, Gc,
             ws_inside, ws_holds);
  CSG_LAUNCH(k_count_fold, dim3((unsigned)cdiv(m + n, 256)), dim3(256), 0, s, (const int*)ws_inside, (int)m, Gc, (int*)inside,
             (const int*)ws_holds, (int)n, Gq, (int*)holds);
  return check_launch("csg_ball_counts");
}

}  // extern "C"
