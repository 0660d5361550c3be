// The passes around the Inception-v3 forward (canonicalsg2im_amd/inception.py) and the statistics behind FID and the
// Inception score (canonicalsg2im_amd/quality.py).  The convolutions themselves are igemm.hip's; everything here is a
// memory-bound pass or a small reduction: 16-byte accesses along the channel axis, no atomics, every sum in one fixed
// order (the same bits on every run).
//
//   k_resize_bilinear   F.interpolate(mode='bilinear', align_corners=False) + a*x + b, fp32 NHWC or uint8 HWC -> NHWC4
//   k_pool3             3x3 max / avg over 9 / avg over the taps inside the picture, (stride, pad) (1,1) or (2,0)
//   k_spatial_mean      (B, P, C) -> (B, C)
//   k_bias_act          y = act(y + bias) on a channel slice: the epilogue of a convolution summed from two launches
//   k_feat_stats        sum += sum_n x[n], outer += sum_n x[n] x[n]^T in fp64; k_feat_finalize: mean and np.cov(ddof=1)
//   k_softmax_rows      row softmax in fp32, stored as fp64 (evaluation/inception.py:28,33)
//   k_is_*              compute_score of evaluation/inception.py:35-49 in fp64
#include <math.h>

#include "csg_common.h"
#include "csg_reduce.h"

namespace csg {

// ------------------------------------------------------------------------------------------------ resize
// One thread per output pixel.  torch's rule (UpSampleKernel, align_corners=False): src = (dst + 0.5) * (in / out) - 0.5,
// clamped at 0; i0 = (int)src, i1 = min(i0 + 1, in - 1), l1 = src - i0, l0 = 1 - l1;
// out = l0y * (l0x * v00 + l1x * v01) + l1y * (l0x * v10 + l1x * v11), then a * out + b.
template <bool U8>
__global__ __launch_bounds__(256) void k_resize_bilinear(const void* __restrict__ src, int B, int IH, int IW, int cs, int OH,
                                                         int OW, float sy, float sx, float a, float b, int reverse,
                                                         float4* __restrict__ out) {
  const int64_t total = (int64_t)B * OH * OW;
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const int ox = (int)(i % OW);
  const int oy = (int)((i / OW) % OH);
  const int64_t img = i / ((int64_t)OW * OH);
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
  const int64_t base = img * IH * IW;
  const int64_t p00 = (base + (int64_t)y0 * IW + x0) * cs, p01 = (base + (int64_t)y0 * IW + x1) * cs;
  const int64_t p10 = (base + (int64_t)y1 * IW + x0) * cs, p11 = (base + (int64_t)y1 * IW + x1) * cs;
  float r[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    float v00, v01, v10, v11;
    if (U8) {
      const uint8_t* s = (const uint8_t*)src;
      v00 = (float)s[p00 + c] / 255.f, v01 = (float)s[p01 + c] / 255.f;
      v10 = (float)s[p10 + c] / 255.f, v11 = (float)s[p11 + c] / 255.f;
    } else {
      const float* s = (const float*)src;
      v00 = s[p00 + c], v01 = s[p01 + c], v10 = s[p10 + c], v11 = s[p11 + c];
    }
    const float v = ly0 * (lx0 * v00 + lx1 * v01) + ly1 * (lx0 * v10 + lx1 * v11);
    r[c] = a * v + b;
  }
  out[i] = reverse ? make_float4(r[2], r[1], r[0], 0.f) : make_float4(r[0], r[1], r[2], 0.f);
}

// ------------------------------------------------------------------------------------------------ 3x3 pool
// One thread per (output pixel, 4 channels).  The taps are visited row by row, left to right, and only those inside
// the picture: max starts from -inf; the averages start from 0 and add the taps in that order, then divide ONCE by 9
// (kind 1) or by the number of taps inside the picture (kind 2) — the operations of torch's host avg_pool2d.
__device__ __forceinline__ float pmax(float m, float v) { return (v > m || v != v) ? v : m; }   // NaN propagates

__global__ __launch_bounds__(256) void k_pool3(const float* __restrict__ x, int B, int H, int W, int C4, int x_cs, int kind,
                                               int stride, int pad, int OH, int OW, float* __restrict__ y, int y_cs,
                                               int y_off) {
  const int64_t total = (int64_t)B * OH * OW * C4;
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const int c = (int)(i % C4) * 4;
  const int64_t pix = i / C4;
  const int ox = (int)(pix % OW);
  const int oy = (int)((pix / OW) % OH);
  const int64_t img = pix / ((int64_t)OW * OH);
  const int ys = oy * stride - pad, xs = ox * stride - pad;
  const float ninf = -INFINITY;
  float4 acc = kind == 0 ? make_float4(ninf, ninf, ninf, ninf) : make_float4(0.f, 0.f, 0.f, 0.f);
  int inside = 0;
  for (int dy = 0; dy < 3; ++dy) {
    const int iy = ys + dy;
    if (iy < 0 || iy >= H) continue;
    for (int dx = 0; dx < 3; ++dx) {
      const int ix = xs + dx;
      if (ix < 0 || ix >= W) continue;
      const float4 v = *(const float4*)(x + ((img * H + iy) * W + ix) * x_cs + c);
      if (kind == 0) {
        acc.x = pmax(acc.x, v.x), acc.y = pmax(acc.y, v.y), acc.z = pmax(acc.z, v.z), acc.w = pmax(acc.w, v.w);
      } else {
        acc.x += v.x, acc.y += v.y, acc.z += v.z, acc.w += v.w;
      }
      ++inside;
    }
  }
  if (kind != 0) {
    const float div = kind == 1 ? 9.f : (float)inside;
    acc.x /= div, acc.y /= div, acc.z /= div, acc.w /= div;
  }
  *(float4*)(y + pix * y_cs + y_off + c) = acc;
}

// ------------------------------------------------------------------------------------------------ spatial mean
// One block per (image, 64 channels): 16 channel quads x 16 pixel lanes; a lane adds its pixels p = lane, lane + 16, ...
// in order, the 16 lanes are summed in lane order, the sum is divided by P.
__global__ __launch_bounds__(256) void k_spatial_mean(const float* __restrict__ x, int P, int C, int x_cs,
                                                      float* __restrict__ y) {
  __shared__ float4 part[16][16];
  const int q = threadIdx.x & 15, lane = threadIdx.x >> 4;
  const int c = (blockIdx.x * 16 + q) * 4;
  const int64_t img = blockIdx.y;
  float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
  if (c < C) {
    for (int p = lane; p < P; p += 16) {
      const float4 v = *(const float4*)(x + (img * P + p) * x_cs + c);
      acc.x += v.x, acc.y += v.y, acc.z += v.z, acc.w += v.w;
    }
  }
  part[lane][q] = acc;
  __syncthreads();
  if (lane == 0 && c < C) {
    for (int l = 1; l < 16; ++l) {
      const float4 v = part[l][q];
      acc.x += v.x, acc.y += v.y, acc.z += v.z, acc.w += v.w;
    }
    const float n = (float)P;
    *(float4*)(y + img * C + c) = make_float4(acc.x / n, acc.y / n, acc.z / n, acc.w / n);
  }
}

// ------------------------------------------------------------------------------------------------ bias + activation
__global__ __launch_bounds__(256) void k_bias_act(float* __restrict__ y, int64_t P, int C4, int y_cs, int y_off,
                                                  const float* __restrict__ bias, int act, float slope) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= P * C4) return;
  const int c = (int)(i % C4) * 4;
  float4* dst = (float4*)(y + (i / C4) * y_cs + y_off + c);
  float4 v = *dst;
  if (bias != nullptr) {
    const float4 bv = *(const float4*)(bias + c);
    v.x += bv.x, v.y += bv.y, v.z += bv.z, v.w += bv.w;
  }
  if (act == CSG_ACT_LEAKY) {
    v.x = v.x > 0.f ? v.x : slope * v.x, v.y = v.y > 0.f ? v.y : slope * v.y;
    v.z = v.z > 0.f ? v.z : slope * v.z, v.w = v.w > 0.f ? v.w : slope * v.w;
  } else if (act == CSG_ACT_TANH) {
    v.x = tanhf(v.x), v.y = tanhf(v.y), v.z = tanhf(v.z), v.w = tanhf(v.w);
  }
  *dst = v;
}

// ------------------------------------------------------------------------------------------------ feature statistics
// One block owns the 64 x 64 tile (ti, tj), ti <= tj, of `outer`; a thread owns 4 x 4 of it in fp64 registers and walks the
// n rows in order (the product of two fp32 values is exact in fp64).  At the end the tile is added to outer and the new
// values are copied to the mirrored tile; the diagonal tiles also own their 64 entries of `sum`.
__global__ __launch_bounds__(256) void k_feat_stats(const float* __restrict__ x, int n, int D, int T, double* __restrict__ sum,
                                                    double* __restrict__ outer) {
  // tile index -> (ti, tj) of the upper triangle, rows in order
  int t = blockIdx.x, ti = 0;
  while (t >= T - ti) {
    t -= T - ti;
    ++ti;
  }
  const int tj = ti + t;
  const int ri = threadIdx.x >> 4, rj = threadIdx.x & 15;
  const int i0 = ti * 64 + ri * 4, j0 = tj * 64 + rj * 4;
  double acc[4][4] = {};
  double s[4] = {0.0, 0.0, 0.0, 0.0};
  for (int r = 0; r < n; ++r) {
    const float4 a = *(const float4*)(x + (int64_t)r * D + i0);
    const float4 b = *(const float4*)(x + (int64_t)r * D + j0);
    const double av[4] = {(double)a.x, (double)a.y, (double)a.z, (double)a.w};
    const double bv[4] = {(double)b.x, (double)b.y, (double)b.z, (double)b.w};
#pragma unroll
    for (int u = 0; u < 4; ++u) {
#pragma unroll
      for (int v = 0; v < 4; ++v) acc[u][v] += av[u] * bv[v];
      s[u] += av[u];
    }
  }
#pragma unroll
  for (int u = 0; u < 4; ++u) {
#pragma unroll
    for (int v = 0; v < 4; ++v) {
      const int64_t up = (int64_t)(i0 + u) * D + j0 + v;
      const double nv = outer[up] + acc[u][v];
      outer[up] = nv;
      if (ti != tj) outer[(int64_t)(j0 + v) * D + i0 + u] = nv;
    }
  }
  if (ti == tj && rj == 0) {
#pragma unroll
    for (int u = 0; u < 4; ++u) sum[i0 + u] += s[u];
  }
}

// mu = sum / N; sigma = (outer - N mu mu^T) / (N - 1)   (np.mean, np.cov(rowvar=False); N = 1 gives 0 / 0 = NaN as numpy)
__global__ __launch_bounds__(256) void k_feat_finalize(const double* __restrict__ sum, const double* __restrict__ outer,
                                                       double N, int D, double* __restrict__ mu, double* __restrict__ sigma) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= (int64_t)D * D) return;
  const int r = (int)(i / D), c = (int)(i % D);
  const double mr = sum[r] / N, mc = sum[c] / N;
  if (c == 0) mu[r] = mr;
  sigma[i] = (outer[i] - N * (mr * mc)) / (N - 1.0);      // mr * mc first: the same bits at (r, c) and (c, r)
}

// ------------------------------------------------------------------------------------------------ softmax, score
__device__ __forceinline__ float block_max_f32(float v, float* part) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v = fmaxf(v, __shfl_down(v, off, 64));
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = v;
  __syncthreads();
  v = fmaxf(fmaxf(part[0], part[1]), fmaxf(part[2], part[3]));
  __syncthreads();
  return v;
}
__device__ __forceinline__ float block_sum_f32(float v, float* part) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = v;
  __syncthreads();
  v = ((part[0] + part[1]) + part[2]) + part[3];
  __syncthreads();
  return v;
}
// thread 0's block_sum_f64 result to every thread
__device__ __forceinline__ double block_total_f64(double v, double (*part)[1], double* bc) {
  double a[1] = {v};
  block_sum_f64<1, 4>(a, part);
  if (threadIdx.x == 0) *bc = a[0];
  __syncthreads();
  const double r = *bc;
  __syncthreads();
  return r;
}

// one block per row: p = exp(x - max) / sum, fp32 arithmetic, stored as fp64
__global__ __launch_bounds__(256) void k_softmax_rows(const float* __restrict__ logits, int K, int64_t ld,
                                                      double* __restrict__ probs) {
  __shared__ float part[4];
  const float* row = logits + (int64_t)blockIdx.x * ld;
  float m = -INFINITY;
  for (int j = threadIdx.x; j < K; j += 256) m = fmaxf(m, row[j]);
  m = block_max_f32(m, part);
  float s = 0.f;
  for (int j = threadIdx.x; j < K; j += 256) s += expf(row[j] - m);
  s = block_sum_f32(s, part);
  for (int j = threadIdx.x; j < K; j += 256) probs[(int64_t)blockIdx.x * K + j] = (double)(expf(row[j] - m) / s);
}

// py[k][j] = mean over the rows of split k, rows in order (grid: (ceil(K / 256), splits))
__global__ __launch_bounds__(256) void k_is_marginal(const double* __restrict__ probs, int per, int K, double* __restrict__ py) {
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j >= K) return;
  const int k = blockIdx.y;
  double s = 0.0;
  for (int r = 0; r < per; ++r) s += probs[((int64_t)k * per + r) * K + j];
  py[(int64_t)k * K + j] = s / (double)per;
}

// kl[i] = scipy.stats.entropy(p_i, py): both renormalised by their sums, sum_j rel_entr(pk_j, qk_j)  (one block per row)
__global__ __launch_bounds__(256) void k_is_kl(const double* __restrict__ probs, const double* __restrict__ py, int per, int K,
                                               double* __restrict__ kl) {
  __shared__ double part[4][1];
  __shared__ double bc;
  const int i = blockIdx.x;
  const double* p = probs + (int64_t)i * K;
  const double* q = py + (int64_t)(i / per) * K;
  double sp = 0.0, sq = 0.0;
  for (int j = threadIdx.x; j < K; j += 256) {
    sp += p[j];
    sq += q[j];
  }
  sp = block_total_f64(sp, part, &bc);
  sq = block_total_f64(sq, part, &bc);
  double acc = 0.0;
  for (int j = threadIdx.x; j < K; j += 256) {
    const double a = p[j] / sp, b = q[j] / sq;
    if (a > 0.0 && b > 0.0)
      acc += a * log(a / b);
    else if (!(a == 0.0 && b >= 0.0))
      acc += INFINITY;
  }
  acc = block_total_f64(acc, part, &bc);
  if (threadIdx.x == 0) kl[i] = acc;
}

// out = [mean, population std, score of split 0, 1, ...]; score_k = exp(mean_i kl_i), rows in order (one wave)
__global__ __launch_bounds__(64) void k_is_fold(const double* __restrict__ kl, int per, int splits, double* __restrict__ out) {
  if (threadIdx.x != 0) return;
  double m = 0.0;
  for (int k = 0; k < splits; ++k) {
    double s = 0.0;
    for (int r = 0; r < per; ++r) s += kl[(int64_t)k * per + r];
    const double sc = exp(s / (double)per);
    out[2 + k] = sc;
    m += sc;
  }
  m /= (double)splits;
  double v = 0.0;
  for (int k = 0; k < splits; ++k) v += (out[2 + k] - m) * (out[2 + k] - m);
  out[0] = m;
  out[1] = sqrt(v / (double)splits);
}

}  // namespace csg

using namespace csg;

extern "C" {

int csg_resize_bilinear(const void* src, int32_t src_u8, int64_t B, int64_t IH, int64_t IW, int64_t src_cs, int64_t OH,
                        int64_t OW, float a, float b, int32_t reverse, float* out, void* stream) {
  CSG_REQUIRE(src != nullptr && out != nullptr, CSG_E_BADSHAPE, "csg_resize_bilinear: null operand");
  CSG_REQUIRE(B > 0 && IH > 0 && IW > 0 && OH > 0 && OW > 0 && IH <= 16384 && IW <= 16384 && OH <= 16384 && OW <= 16384,
              CSG_E_BADSHAPE, "csg_resize_bilinear: sides must be in 1..16384");
  CSG_REQUIRE(src_u8 ? src_cs == 3 : (src_cs == 3 || src_cs == 4), CSG_E_UNSUPPORTED,
              "csg_resize_bilinear: %d values per source pixel (uint8: 3; fp32: 3 or 4)", (int)src_cs);
  CSG_REQUIRE(B * IH * IW < (1ll << 31) && B * OH * OW < (1ll << 31), CSG_E_UNSUPPORTED, "csg_resize_bilinear: too many pixels");
  CSG_REQUIRE((uintptr_t)out % 16 == 0 && (src_u8 || (uintptr_t)src % 4 == 0), CSG_E_BADSHAPE,
              "csg_resize_bilinear: out must be 16-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  const int64_t total = B * OH * OW;
  const float sy = (float)IH / (float)OH, sx = (float)IW / (float)OW;
  ProfScope p(K_RESIZE_BILINEAR, (double)total * (16 + 12.0 * (src_u8 ? 1 : 4)), s);
  if (src_u8)
    CSG_LAUNCH(k_resize_bilinear<true>, dim3((unsigned)cdiv(total, 256)), dim3(256), 0, s, src, (int)B, (int)IH, (int)IW,
               (int)src_cs, (int)OH, (int)OW, sy, sx, a, b, (int)reverse, (float4*)out);
  else
    CSG_LAUNCH(k_resize_bilinear<false>, dim3((unsigned)cdiv(total, 256)), dim3(256), 0, s, src, (int)B, (int)IH, (int)IW,
               (int)src_cs, (int)OH, (int)OW, sy, sx, a, b, (int)reverse, (float4*)out);
  return check_launch("csg_resize_bilinear");
}

int csg_pool3(const float* x, int64_t B, int64_t H, int64_t W, int64_t C, int64_t x_cs, int32_t kind, int32_t stride,
              int32_t pad, float* y, int64_t y_cs, int64_t y_off, void* stream) {
  CSG_REQUIRE(x != nullptr && y != nullptr, CSG_E_BADSHAPE, "csg_pool3: null operand");
  CSG_REQUIRE(kind >= 0 && kind <= 2, CSG_E_UNSUPPORTED, "csg_pool3: kind %d (0 max, 1 avg over 9, 2 avg over the taps inside)",
              (int)kind);
  CSG_REQUIRE((stride == 1 && pad == 1) || (stride == 2 && pad == 0), CSG_E_UNSUPPORTED,
              "csg_pool3: (stride, pad) = (%d, %d); served: (1, 1) and (2, 0)", (int)stride, (int)pad);
  CSG_REQUIRE(B > 0 && H > 0 && W > 0 && C > 0 && H + 2 * pad >= 3 && W + 2 * pad >= 3, CSG_E_BADSHAPE,
              "csg_pool3: bad shape B=%ld H=%ld W=%ld C=%ld", (long)B, (long)H, (long)W, (long)C);
  CSG_REQUIRE(C % 4 == 0 && x_cs % 4 == 0 && y_cs % 4 == 0 && y_off % 4 == 0 && x_cs >= C && y_off >= 0 && y_off + C <= y_cs,
              CSG_E_BADSHAPE, "csg_pool3: C, x_cs, y_cs, y_off must be multiples of 4 with C <= x_cs and y_off + C <= y_cs");
  CSG_REQUIRE(((uintptr_t)x | (uintptr_t)y) % 16 == 0, CSG_E_BADSHAPE, "csg_pool3: x and y must be 16-byte aligned");
  const int64_t OH = (H + 2 * pad - 3) / stride + 1, OW = (W + 2 * pad - 3) / stride + 1;
  CSG_REQUIRE(B * H * W * x_cs < (1ll << 40) && B * OH * OW * (C / 4) < (1ll << 40) && H < (1 << 20) && W < (1 << 20) &&
                  x_cs < (1 << 20) && y_cs < (1 << 20),
              CSG_E_UNSUPPORTED, "csg_pool3: map too large");
  hipStream_t s = (hipStream_t)stream;
  const int64_t total = B * OH * OW * (C / 4);
  CSG_REQUIRE(cdiv(total, 256) < (1ll << 31), CSG_E_UNSUPPORTED, "csg_pool3: map too large");
  ProfScope p(K_POOL3, (double)B * (H * W + OH * OW) * C * 4, s);
  CSG_LAUNCH(k_pool3, dim3((unsigned)cdiv(total, 256)), dim3(256), 0, s, x, (int)B, (int)H, (int)W, (int)(C / 4), (int)x_cs,
             (int)kind, (int)stride, (int)pad, (int)OH, (int)OW, y, (int)y_cs, (int)y_off);
  return check_launch("csg_pool3");
}

int csg_spatial_mean(const float* x, int64_t B, int64_t P, int64_t C, int64_t x_cs, float* y, void* stream) {
  CSG_REQUIRE(x != nullptr && y != nullptr, CSG_E_BADSHAPE, "csg_spatial_mean: null operand");
  CSG_REQUIRE(B > 0 && B <= 65535 && P > 0 && P < (1 << 24) && C > 0 && C % 4 == 0 && x_cs % 4 == 0 && x_cs >= C &&
                  x_cs < (1 << 20),
              CSG_E_BADSHAPE, "csg_spatial_mean: bad shape B=%ld P=%ld C=%ld x_cs=%ld", (long)B, (long)P, (long)C, (long)x_cs);
  CSG_REQUIRE(((uintptr_t)x | (uintptr_t)y) % 16 == 0, CSG_E_BADSHAPE, "csg_spatial_mean: x and y must be 16-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  ProfScope p(K_SPATIAL_MEAN, (double)B * (P + 1) * C * 4, s);
  CSG_LAUNCH(k_spatial_mean, dim3((unsigned)cdiv(C, 64), (unsigned)B), dim3(256), 0, s, x, (int)P, (int)C, (int)x_cs, y);
  return check_launch("csg_spatial_mean");
}

int csg_bias_act(float* y, int64_t P, int64_t C, int64_t y_cs, int64_t y_off, const float* bias, int32_t act, float slope,
                 void* stream) {
  CSG_REQUIRE(y != nullptr, CSG_E_BADSHAPE, "csg_bias_act: null operand");
  CSG_REQUIRE(P > 0 && C > 0 && C % 4 == 0 && y_cs % 4 == 0 && y_off % 4 == 0 && y_off >= 0 && y_off + C <= y_cs &&
                  y_cs < (1 << 20) && P < (1ll << 31),
              CSG_E_BADSHAPE, "csg_bias_act: bad shape P=%ld C=%ld y_cs=%ld y_off=%ld", (long)P, (long)C, (long)y_cs, (long)y_off);
  CSG_REQUIRE(act == CSG_ACT_NONE || act == CSG_ACT_LEAKY || act == CSG_ACT_TANH, CSG_E_UNSUPPORTED, "csg_bias_act: act %d",
              (int)act);
  CSG_REQUIRE((uintptr_t)y % 16 == 0 && (uintptr_t)bias % 16 == 0, CSG_E_BADSHAPE, "csg_bias_act: y and bias must be 16-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  const int64_t total = P * (C / 4);
  ProfScope p(K_BIAS_ACT, (double)P * C * 8, s);
  CSG_LAUNCH(k_bias_act, dim3((unsigned)cdiv(total, 256)), dim3(256), 0, s, y, P, (int)(C / 4), (int)y_cs, (int)y_off, bias,
             (int)act, slope);
  return check_launch("csg_bias_act");
}

int csg_feat_stats(const float* x, int64_t n, int64_t D, double* sum, double* outer, void* stream) {
  CSG_REQUIRE(x != nullptr && sum != nullptr && outer != nullptr, CSG_E_BADSHAPE, "csg_feat_stats: null operand");
  CSG_REQUIRE(n > 0 && n < (1 << 24) && D > 0 && D % 64 == 0 && D <= 8192, CSG_E_BADSHAPE,
              "csg_feat_stats: n=%ld, D=%ld (D a multiple of 64, at most 8192)", (long)n, (long)D);
  CSG_REQUIRE((uintptr_t)x % 16 == 0 && ((uintptr_t)sum | (uintptr_t)outer) % 8 == 0, CSG_E_BADSHAPE,
              "csg_feat_stats: x must be 16-byte aligned, the fp64 buffers 8-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  const int T = (int)(D / 64);
  ProfScope p(K_FEAT_STATS, (double)D * D * 16 + (double)n * D * 4, s);
  CSG_LAUNCH(k_feat_stats, dim3((unsigned)(T * (T + 1) / 2)), dim3(256), 0, s, x, (int)n, (int)D, T, sum, outer);
  return check_launch("csg_feat_stats");
}

int csg_feat_stats_finalize(const double* sum, const double* outer, int64_t N, int64_t D, double* mu, double* sigma,
                            void* stream) {
  CSG_REQUIRE(sum != nullptr && outer != nullptr && mu != nullptr && sigma != nullptr, CSG_E_BADSHAPE,
              "csg_feat_stats_finalize: null operand");
  CSG_REQUIRE(N >= 1 && D > 0 && D <= 8192, CSG_E_BADSHAPE, "csg_feat_stats_finalize: N=%ld, D=%ld", (long)N, (long)D);
  hipStream_t s = (hipStream_t)stream;
  ProfScope p(K_FEAT_STATS, (double)D * D * 16, s);
  CSG_LAUNCH(k_feat_finalize, dim3((unsigned)cdiv(D * D, 256)), dim3(256), 0, s, sum, outer, (double)N, (int)D, mu, sigma);
  return check_launch("csg_feat_stats_finalize");
}

int csg_softmax_rows(const float* logits, int64_t N, int64_t K, int64_t ld, double* probs, void* stream) {
  CSG_REQUIRE(logits != nullptr && probs != nullptr, CSG_E_BADSHAPE, "csg_softmax_rows: null operand");
  CSG_REQUIRE(N > 0 && N < (1ll << 31) && K > 0 && K <= (1 << 20) && ld >= K, CSG_E_BADSHAPE,
              "csg_softmax_rows: N=%ld K=%ld ld=%ld", (long)N, (long)K, (long)ld);
  hipStream_t s = (hipStream_t)stream;
  ProfScope p(K_INCEPTION_SCORE, (double)N * K * 12, s);
  CSG_LAUNCH(k_softmax_rows, dim3((unsigned)N), dim3(256), 0, s, logits, (int)K, ld, probs);
  return check_launch("csg_softmax_rows");
}

int64_t csg_inception_score_workspace(int64_t N, int64_t K, int64_t splits) {
  if (N <= 0 || K <= 0 || splits <= 0 || splits > N) return -1;
  return (splits * K + N) * 8;
}

int csg_inception_score(const double* probs, int64_t N, int64_t K, int64_t splits, double* workspace, int64_t workspace_bytes,
                        double* out, void* stream) {
  CSG_REQUIRE(probs != nullptr && workspace != nullptr && out != nullptr, CSG_E_BADSHAPE, "csg_inception_score: null operand");
  CSG_REQUIRE(N > 0 && N < (1ll << 31) && K > 0 && K <= (1 << 20) && splits >= 1 && splits <= 65535 && splits <= N,
              CSG_E_BADSHAPE, "csg_inception_score: N=%ld K=%ld splits=%ld (1 <= splits <= N)", (long)N, (long)K, (long)splits);
  CSG_REQUIRE(workspace_bytes >= csg_inception_score_workspace(N, K, splits), CSG_E_WORKSPACE,
              "csg_inception_score: needs %lld bytes of workspace", (long long)csg_inception_score_workspace(N, K, splits));
  hipStream_t s = (hipStream_t)stream;
  const int per = (int)(N / splits);       // the reference drops the rows behind splits * (N // splits)
  double* py = workspace;
  double* kl = workspace + splits * K;
  ProfScope p(K_INCEPTION_SCORE, (double)splits * per * K * 24, s);
  CSG_LAUNCH(k_is_marginal, dim3((unsigned)cdiv(K, 256), (unsigned)splits), dim3(256), 0, s, probs, per, (int)K, py);
  CSG_LAUNCH(k_is_kl, dim3((unsigned)(splits * per)), dim3(256), 0, s, probs, (const double*)py, per, (int)K, kl);
  CSG_LAUNCH(k_is_fold, dim3(1), dim3(64), 0, s, (const double*)kl, per, (int)splits, out);
  return check_launch("csg_inception_score");
}

}  // extern "C"
