// The passes behind KID and the object-level FID (canonicalsg2im_amd/quality.py): the crop stage in front of the Inception
// network and the fp64 sums behind the two numbers.  As in inception.hip: no atomics, every sum in one fixed order (the same
// bits on every run), stream ordered, nothing read back.
//
//   k_crop_windows          boxes (N,4) fp32 xywh in units of the picture -> integer pixel windows [X0, Y0, X1, Y1)
//   k_crop_resize_bilinear  "cut the window out, then k_resize_bilinear it" over all crops at once, uint8 HWC -> NHWC4
//   k_kid_tiles / _fold     the three polynomial-kernel sums of KID for S subsets, 64 x 64 tiles, no Gram matrix in memory
//   k_feat_class_sums       per-class fp64 sums of feature rows
#include <math.h>

#include "csg_common.h"
#include "csg_reduce.h"

namespace csg {

// ------------------------------------------------------------------------------------------------ windows
// The guarded conversion: a value that is not >= 0 (negative, NaN) gives 0, a value above `side` (+inf included) gives
// `side`; what is left lies in [0, side] and the cast is defined.
__device__ __forceinline__ int guarded_int(float v, int side) {
  if (!(v >= 0.f)) return 0;
  if (v > (float)side) return side;
  return (int)v;
}

// fx0 = x * W, fx1 = (x + w) * W, one fp32 operation each; X0 = clamp(floor(fx0), 0, W - 1), X1 = clamp(ceil(fx1), X0 + 1, W)
__global__ __launch_bounds__(256) void k_crop_windows(const float4* __restrict__ boxes, int N, int H, int W,
                                                      int4* __restrict__ win) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= N) return;
  const float4 b = boxes[i];
  const float fx0 = b.x * (float)W, fx1 = (b.x + b.z) * (float)W;
  const float fy0 = b.y * (float)H, fy1 = (b.y + b.w) * (float)H;
  int X0 = guarded_int(floorf(fx0), W), Y0 = guarded_int(floorf(fy0), H);
  X0 = X0 > W - 1 ? W - 1 : X0;
  Y0 = Y0 > H - 1 ? H - 1 : Y0;
  int X1 = guarded_int(ceilf(fx1), W), Y1 = guarded_int(ceilf(fy1), H);
  X1 = X1 < X0 + 1 ? X0 + 1 : X1;
  Y1 = Y1 < Y0 + 1 ? Y0 + 1 : Y1;
  win[i] = make_int4(X0, Y0, X1, Y1);
}

// ------------------------------------------------------------------------------------------------ crop + resize
// One thread per output pixel.  k_resize_bilinear<true>'s arithmetic (inception.hip), expression for expression, with the
// window standing for the whole picture: the taps are clamped to the window, then offset by (Y0, X0).  The window and the
// picture's index are clamped once more in integers before an address is formed: whatever the two arrays hold, every read
// lies inside `pics`.
__global__ __launch_bounds__(256) void k_crop_resize_bilinear(const uint8_t* __restrict__ pics, int B, int H, int W,
                                                              const int4* __restrict__ win, const int* __restrict__ image_index,
                                                              int N, int OH, int OW, float a, float b, int reverse,
                                                              float4* __restrict__ out) {
  const int64_t total = (int64_t)N * OH * OW;
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const int ox = (int)(i % OW);
  const int oy = (int)((i / OW) % OH);
  const int n = (int)(i / ((int64_t)OW * OH));
  int4 w = win[n];
  w.x = w.x < 0 ? 0 : (w.x > W - 1 ? W - 1 : w.x);
  w.y = w.y < 0 ? 0 : (w.y > H - 1 ? H - 1 : w.y);
  w.z = w.z < w.x + 1 ? w.x + 1 : (w.z > W ? W : w.z);
  w.w = w.w < w.y + 1 ? w.y + 1 : (w.w > H ? H : w.w);
  int64_t img = image_index[n];
  img = img < 0 ? 0 : (img > B - 1 ? B - 1 : img);
  const int IH = w.w - w.y, IW = w.z - w.x;
  const float sy = (float)IH / (float)OH, sx = (float)IW / (float)OW;
  float fy = ((float)oy + 0.5f) * sy - 0.5f;
  float fx = ((float)ox + 0.5f) * sx - 0.5f;
  fy = fy < 0.f ? 0.f : fy;
  fx = fx < 0.f ? 0.f : fx;
  int y0 = (int)fy, x0 = (int)fx;
  y0 = y0 > IH - 1 ? IH - 1 : y0;
  x0 = x0 > IW - 1 ? IW - 1 : x0;
  const int y1 = y0 + 1 > IH - 1 ? IH - 1 : y0 + 1;
  const int x1 = x0 + 1 > IW - 1 ? IW - 1 : x0 + 1;
  const float ly1 = fy - (float)y0, lx1 = fx - (float)x0;
  const float ly0 = 1.f - ly1, lx0 = 1.f - lx1;
  const int64_t base = img * H * W;
  const int64_t p00 = (base + (int64_t)(w.y + y0) * W + w.x + x0) * 3, p01 = (base + (int64_t)(w.y + y0) * W + w.x + x1) * 3;
  const int64_t p10 = (base + (int64_t)(w.y + y1) * W + w.x + x0) * 3, p11 = (base + (int64_t)(w.y + y1) * W + w.x + x1) * 3;
  float r[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const float v00 = (float)pics[p00 + c] / 255.f, v01 = (float)pics[p01 + c] / 255.f;
    const float v10 = (float)pics[p10 + c] / 255.f, v11 = (float)pics[p11 + c] / 255.f;
    const float v = ly0 * (lx0 * v00 + lx1 * v01) + ly1 * (lx0 * v10 + lx1 * v11);
    r[c] = a * v + b;
  }
  out[i] = reverse ? make_float4(r[2], r[1], r[0], 0.f) : make_float4(r[0], r[1], r[2], 0.f);
}

// ------------------------------------------------------------------------------------------------ KID
// Per subset the tiles are numbered: the T (T + 1) / 2 upper-triangle tiles of xx (rows in order), those of yy, then the
// T x T tiles of xy.  A block owns one 64 x 64 tile: the two 64-row operands are staged KD feature columns at a time into
// LDS, transposed ([column][row]), read through the subset's index arrays — a row past m is staged as zeros and never
// addressed.  A thread owns 4 x 4 dot products in fp64 registers and walks the columns in order (the product of two fp32
// values is exact in fp64).  Then k = (gamma dot + coef0)^degree per entry inside the subset, i != j on the diagonal tiles
// of xx and yy, the 16 entries added row by row, the block's 256 sums by block_sum_f64's fixed tree, an off-diagonal
// tile of xx or yy doubled (exact).  k_kid_fold adds a matrix's tiles in index order.
constexpr int kKidKD = 32;        // feature columns per stage: 2 x 32 x 68 floats = 17 KB of LDS
constexpr int kKidLD = 68;        // 64 rows + 4: a stage row starts on a 16-byte boundary

__host__ __device__ static inline int64_t kid_tiles_per_subset(int64_t T) { return T * (T + 1) + T * T; }

__global__ __launch_bounds__(256) void k_kid_tiles(const float* __restrict__ fx, const float* __restrict__ fy, int nx, int ny,
                                                   int D, const int* __restrict__ ix, const int* __restrict__ iy, int m, int T,
                                                   double gamma, double coef0, int degree, double* __restrict__ ws) {
  __shared__ __attribute__((aligned(16))) float As[kKidKD][kKidLD];
  __shared__ __attribute__((aligned(16))) float Bs[kKidKD][kKidLD];
  __shared__ double part[4][1];
  const int s = blockIdx.y;
  const int tri = T * (T + 1) / 2;
  int t = blockIdx.x, which, ti, tj;
  if (t < 2 * tri) {
    which = t >= tri ? 1 : 0;
    t -= which * tri;
    ti = 0;
    while (t >= T - ti) {
      t -= T - ti;
      ++ti;
    }
    tj = ti + t;
  } else {
    which = 2;
    t -= 2 * tri;
    ti = t / T;
    tj = t % T;
  }
  const float* A = which == 1 ? fy : fx;
  const float* Bm = which == 0 ? fx : fy;
  const int nA = which == 1 ? ny : nx, nB = which == 0 ? nx : ny;
  const int* idA = (which == 1 ? iy : ix) + (int64_t)s * m;
  const int* idB = (which == 0 ? ix : iy) + (int64_t)s * m;
  // staging role: rows lr and lr + 32 of both operands, the column quad q
  const int lr = threadIdx.x >> 3, q = threadIdx.x & 7;
  int64_t ra[2], rb[2];
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const int gi = ti * 64 + lr + 32 * h, gj = tj * 64 + lr + 32 * h;
    ra[h] = rb[h] = -1;
    if (gi < m) {
      const int r = idA[gi];
      ra[h] = (int64_t)(r < 0 ? 0 : (r > nA - 1 ? nA - 1 : r)) * D + q * 4;
    }
    if (gj < m) {
      const int r = idB[gj];
      rb[h] = (int64_t)(r < 0 ? 0 : (r > nB - 1 ? nB - 1 : r)) * D + q * 4;
    }
  }
  const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
  float4 va[2], vb[2];
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    va[h] = ra[h] >= 0 ? *(const float4*)(A + ra[h]) : zero;
    vb[h] = rb[h] >= 0 ? *(const float4*)(Bm + rb[h]) : zero;
  }
  const int ri = threadIdx.x >> 4, rj = threadIdx.x & 15;
  double acc[4][4] = {};
  for (int k0 = 0; k0 < D; k0 += kKidKD) {
    __syncthreads();
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int row = lr + 32 * h;
      As[q * 4 + 0][row] = va[h].x, As[q * 4 + 1][row] = va[h].y, As[q * 4 + 2][row] = va[h].z, As[q * 4 + 3][row] = va[h].w;
      Bs[q * 4 + 0][row] = vb[h].x, Bs[q * 4 + 1][row] = vb[h].y, Bs[q * 4 + 2][row] = vb[h].z, Bs[q * 4 + 3][row] = vb[h].w;
    }
    __syncthreads();
    if (k0 + kKidKD < D) {      // the next stage's rows travel while this one is multiplied
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        va[h] = ra[h] >= 0 ? *(const float4*)(A + ra[h] + k0 + kKidKD) : zero;
        vb[h] = rb[h] >= 0 ? *(const float4*)(Bm + rb[h] + k0 + kKidKD) : zero;
      }
    }
#pragma unroll 8
    for (int d = 0; d < kKidKD; ++d) {
      const float4 a = *(const float4*)&As[d][ri * 4];
      const float4 b = *(const float4*)&Bs[d][rj * 4];
      const double av[4] = {(double)a.x, (double)a.y, (double)a.z, (double)a.w};
      const double bv[4] = {(double)b.x, (double)b.y, (double)b.z, (double)b.w};
#pragma unroll
      for (int u = 0; u < 4; ++u) {
#pragma unroll
        for (int v = 0; v < 4; ++v) acc[u][v] += av[u] * bv[v];
      }
    }
  }
  double sum[1] = {0.0};
#pragma unroll
  for (int u = 0; u < 4; ++u) {
#pragma unroll
    for (int v = 0; v < 4; ++v) {
      const int gi = ti * 64 + ri * 4 + u, gj = tj * 64 + rj * 4 + v;
      if (gi < m && gj < m && !(which < 2 && gi == gj)) {
        const double p = gamma * acc[u][v] + coef0;
        sum[0] += degree == 1 ? p : (degree == 2 ? p * p : p * p * p);
      }
    }
  }
  block_sum_f64<1, 4>(sum, part);
  if (threadIdx.x == 0) ws[(int64_t)s * kid_tiles_per_subset(T) + blockIdx.x] = (which < 2 && ti != tj) ? 2.0 * sum[0] : sum[0];
}

// out[s][k] = the tiles of matrix k of subset s, added in index order (one wave per subset, lanes 0..2 at work)
__global__ __launch_bounds__(64) void k_kid_fold(const double* __restrict__ ws, int T, double* __restrict__ out) {
  const int k = threadIdx.x;
  if (k >= 3) return;
  const int tri = T * (T + 1) / 2;
  const int64_t per = kid_tiles_per_subset(T);
  const int64_t lo = k == 0 ? 0 : (k == 1 ? tri : 2 * tri), hi = k == 0 ? tri : (k == 1 ? 2 * tri : per);
  const double* w = ws + (int64_t)blockIdx.x * per;
  double s = 0.0;
  for (int64_t t = lo; t < hi; ++t) s += w[t];
  out[(int64_t)blockIdx.x * 3 + k] = s;
}

// ------------------------------------------------------------------------------------------------ per-class sums
// One block per (64-column slab, class): a thread owns one column and walks the n rows in order; the block of slab 0 owns
// the class's count.  An id outside [0, C) matches no block.
__global__ __launch_bounds__(64) void k_feat_class_sums(const float* __restrict__ x, const int* __restrict__ ids, int n, int D,
                                                        double* __restrict__ sums, int64_t* __restrict__ counts) {
  const int c = blockIdx.y;
  const int col = blockIdx.x * 64 + threadIdx.x;
  double acc = 0.0;
  int64_t cnt = 0;
  for (int r = 0; r < n; ++r) {
    if (ids[r] != c) continue;
    acc += (double)x[(int64_t)r * D + col];
    ++cnt;
  }
  if (cnt == 0) return;
  sums[(int64_t)c * D + col] += acc;
  if (col == 0) counts[c] += cnt;
}

}  // namespace csg

using namespace csg;

extern "C" {

int csg_crop_windows(const float* boxes, int64_t N, int64_t H, int64_t W, int32_t* windows, void* stream) {
  CSG_REQUIRE(boxes != nullptr && windows != nullptr, CSG_E_BADSHAPE, "csg_crop_windows: null operand");
  CSG_REQUIRE(N > 0 && N < (1ll << 31) - 256 && H > 0 && W > 0 && H <= 16384 && W <= 16384, CSG_E_BADSHAPE,
              "csg_crop_windows: N=%ld H=%ld W=%ld (N >= 1; sides in 1..16384)", (long)N, (long)H, (long)W);
  CSG_REQUIRE(((uintptr_t)boxes | (uintptr_t)windows) % 16 == 0, CSG_E_BADSHAPE,
              "csg_crop_windows: boxes and windows must be 16-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  ProfScope p(K_CROP_WINDOWS, (double)N * 32, s);
  CSG_LAUNCH(k_crop_windows, dim3((unsigned)cdiv(N, 256)), dim3(256), 0, s, (const float4*)boxes, (int)N, (int)H, (int)W,
             (int4*)windows);
  return check_launch("csg_crop_windows");
}

int csg_crop_resize_bilinear(const uint8_t* pictures, int64_t B, int64_t H, int64_t W, const int32_t* windows,
                             const int32_t* image_index, int64_t N, int64_t OH, int64_t OW, float a, float b, int32_t reverse,
                             float* out, void* stream) {
  CSG_REQUIRE(pictures != nullptr && windows != nullptr && image_index != nullptr && out != nullptr, CSG_E_BADSHAPE,
              "csg_crop_resize_bilinear: null operand");
  CSG_REQUIRE(B > 0 && N > 0 && H > 0 && W > 0 && OH > 0 && OW > 0 && H <= 16384 && W <= 16384 && OH <= 16384 && OW <= 16384,
              CSG_E_BADSHAPE, "csg_crop_resize_bilinear: B and N must be positive, sides in 1..16384");
  CSG_REQUIRE(B * H * W < (1ll << 31) && N * OH * OW < (1ll << 31), CSG_E_UNSUPPORTED, "csg_crop_resize_bilinear: too many pixels");
  CSG_REQUIRE(((uintptr_t)out | (uintptr_t)windows) % 16 == 0 && (uintptr_t)image_index % 4 == 0, CSG_E_BADSHAPE,
              "csg_crop_resize_bilinear: out and windows must be 16-byte aligned, image_index 4-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  const int64_t total = N * OH * OW;
  ProfScope p(K_CROP_RESIZE_BILINEAR, (double)total * (16 + 12.0), s);
  CSG_LAUNCH(k_crop_resize_bilinear, dim3((unsigned)cdiv(total, 256)), dim3(256), 0, s, pictures, (int)B, (int)H, (int)W,
             (const int4*)windows, (const int*)image_index, (int)N, (int)OH, (int)OW, a, b, (int)reverse, (float4*)out);
  return check_launch("csg_crop_resize_bilinear");
}

int64_t csg_kid_sums_workspace_bytes(int64_t S, int64_t m) {
  if (S <= 0 || S > 65535 || m < 2 || m > 65536) return -1;
  return S * kid_tiles_per_subset(cdiv(m, 64)) * 8;
}

int csg_kid_sums(const float* fx, int64_t nx, const float* fy, int64_t ny, int64_t D, const int32_t* ix, const int32_t* iy,
                 int64_t S, int64_t m, double gamma, double coef0, int32_t degree, void* workspace, int64_t workspace_bytes,
                 double* out, void* stream) {
  CSG_REQUIRE(fx != nullptr && fy != nullptr && ix != nullptr && iy != nullptr && workspace != nullptr && out != nullptr,
              CSG_E_BADSHAPE, "csg_kid_sums: null operand");
  CSG_REQUIRE(m >= 2 && m <= 65536, CSG_E_BADSHAPE, "csg_kid_sums: a subset needs 2 .. 65536 rows, got m=%ld", (long)m);
  CSG_REQUIRE(S > 0 && S <= 65535 && nx > 0 && ny > 0 && nx < (1ll << 31) && ny < (1ll << 31) && D > 0 && D % 64 == 0 && D <= 8192,
              CSG_E_BADSHAPE, "csg_kid_sums: S=%ld nx=%ld ny=%ld D=%ld (1 <= S <= 65535; D a multiple of 64, at most 8192)",
              (long)S, (long)nx, (long)ny, (long)D);
  CSG_REQUIRE(degree >= 1 && degree <= 3, CSG_E_UNSUPPORTED, "csg_kid_sums: degree %d (served: 1, 2, 3)", (int)degree);
  CSG_REQUIRE(((uintptr_t)fx | (uintptr_t)fy) % 16 == 0 && ((uintptr_t)ix | (uintptr_t)iy) % 4 == 0 &&
                  ((uintptr_t)workspace | (uintptr_t)out) % 8 == 0,
              CSG_E_BADSHAPE, "csg_kid_sums: features must be 16-byte aligned, indices 4-byte, workspace and out 8-byte aligned");
  CSG_REQUIRE(workspace_bytes >= csg_kid_sums_workspace_bytes(S, m), CSG_E_WORKSPACE, "csg_kid_sums: needs %lld bytes of workspace",
              (long long)csg_kid_sums_workspace_bytes(S, m));
  hipStream_t s = (hipStream_t)stream;
  const int T = (int)cdiv(m, 64);
  const int64_t per = kid_tiles_per_subset(T);
  ProfScope p(K_KID_SUMS, (double)S * per * 64 * 64 * D * 2, s);      // the fp64 multiply-adds of the tiles
  CSG_LAUNCH(k_kid_tiles, dim3((unsigned)per, (unsigned)S), dim3(256), 0, s, fx, fy, (int)nx, (int)ny, (int)D, (const int*)ix,
             (const int*)iy, (int)m, T, gamma, coef0, (int)degree, (double*)workspace);
  CSG_LAUNCH(k_kid_fold, dim3((unsigned)S), dim3(64), 0, s, (const double*)workspace, T, out);
  return check_launch("csg_kid_sums");
}

int csg_feat_class_sums(const float* x, const int32_t* class_ids, int64_t n, int64_t D, int64_t C, double* sums, int64_t* counts,
                        void* stream) {
  CSG_REQUIRE(x != nullptr && class_ids != nullptr && sums != nullptr && counts != nullptr, CSG_E_BADSHAPE,
              "csg_feat_class_sums: null operand");
  CSG_REQUIRE(n > 0 && n < (1 << 24) && D > 0 && D % 64 == 0 && D <= 8192 && C > 0 && C <= 65535, CSG_E_BADSHAPE,
              "csg_feat_class_sums: n=%ld D=%ld C=%ld (D a multiple of 64, at most 8192; 1 <= C <= 65535)", (long)n, (long)D,
              (long)C);
  CSG_REQUIRE((uintptr_t)x % 4 == 0 && (uintptr_t)class_ids % 4 == 0 && ((uintptr_t)sums | (uintptr_t)counts) % 8 == 0,
              CSG_E_BADSHAPE, "csg_feat_class_sums: x and class_ids must be 4-byte aligned, sums and counts 8-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  ProfScope p(K_FEAT_CLASS_SUMS, (double)n * D * 4 + (double)C * D * 16, s);
  CSG_LAUNCH(k_feat_class_sums, dim3((unsigned)(D / 64), (unsigned)C), dim3(64), 0, s, x, (const int*)class_ids, (int)n, (int)D,
             sums, counts);
  return check_launch("csg_feat_class_sums");
}

}  // extern "C"
