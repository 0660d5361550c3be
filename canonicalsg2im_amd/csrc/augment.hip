// DiffAugment (Zhao et al., NeurIPS 2020) of what the discriminators see: colour, translation and cutout of an NHWC map with
// a padded channel count, forward and adjoint, and the parameter table both read (include/csg_hip.h, "DiffAugment").
//
// One sample x of shape (H, H, Ct), colour channels [c0, c0 + 3), row (b, s, c, tx, ty, y0, x0, size) of the table:
//     colour       x1 = x + b;  x2 = (x1 - mp) * s + mp, mp = the pixel's mean of the 3 channels;  x3 = (x2 - mu) * c + mu,
//                  mu = mean over the sample's 3 H H colour values of x, + b (saturation keeps the channel mean)
//     translation  out[y, x] = in[y - ty, x - tx], zero outside, all Ct channels
//     cutout       rows [y0, y0 + size) x columns [x0, x0 + size) of the translated map are zero, all Ct channels
// in that order.  A policy that is off is skipped, not run with identity parameters: with colour off the colour channels are
// bit copies, and what translation and cutout do is copies and +0.0 only.  The map is linear in x, so the backward needs the
// table alone:   g3 = shift back(mask * g);  g2 = c g3 + (1 - c) mean_chw(g3);  gx = s g2 + (1 - s) mean_c(g2)  on the colour
// channels, gx = g3 on the others.
//
// THE fp32 OPERATION SEQUENCE OF THE COLOUR MAP (the contract tests/augment_cases.py derives its bound from; compiled with
// -ffp-contract=off, every fused multiply-add written out).  Forward, per pixel, k = 0..2:
//     x1_k = x_k + b                                   3 additions
//     t = (x1_0 + x1_1) + x1_2;  mp = t / 3            2 additions, 1 division (correctly rounded)
//     d_k = x1_k - mp;  x2_k = fmaf(d_k, s, mp)        1 subtraction, 1 fused multiply-add
//     e_k = x2_k - mu;  x3_k = fmaf(e_k, c, mu)        1 subtraction, 1 fused multiply-add
//     mu = (float)(S / (3 H H) + (double)b)            S: the fp64 sum below; ONE rounding to fp32
// -> 11 roundings feed an output value.  Backward, per pixel (g3_k: the shifted, masked gradient):
//     omc = 1 - c;  q = omc * gbar;  g2_k = fmaf(c, g3_k, q)
//     t = (g2_0 + g2_1) + g2_2;  mg = t / 3;  oms = 1 - s;  r = oms * mg;  gx_k = fmaf(s, g2_k, r)
//     gbar = (float)(S' / (3 H H))                     S': the fp64 sum of g3's colour values
// -> 12 roundings (gbar, omc, q, three g2, two additions, the division, oms, r, gx).
//
// REDUCTIONS.  The per-sample sum is a FIXED tree in fp64 (the fp64 rate is a quarter of the fp32 rate on this part and the
// pass is memory bound; manifold.hip leans on it the same way).  A sample's H H pixels are cut into chunks of CSG_AUG_CHUNK
// = 256 pixels; a thread adds its pixel's three values ((r + g) + b in fp64), a block of 256 lanes sums them with a shuffle
// tree per wave and the four waves in wave order, and writes ONE partial per chunk.  A second, small launch — one block per
// sample — adds the partials: lane l takes chunks l, l + 256, ... in ascending order, then the same block tree, and the
// mean is rounded once to fp32.  The tree depends on (H, the data) alone: the first launch has min(N chunks, 2048) blocks
// that stride over the chunks, and whatever the grid the bits are the same.  No atomics.  At N = 16, H = 256 there are
// 4096 chunks: eight blocks per CU on 256 CUs.
//
// THE MAIN PASS moves 16 bytes per lane and access (csg_vec4.h): one lane owns one float4 of an output pixel row, four of
// them per thread with every load issued before the first store; consecutive lanes write consecutive addresses.  A lane
// whose float4 holds a colour channel fetches the pixel's colour triple again (one or two more 16-byte loads that hit L1 /
// L2).  Nothing that varies per step is a kernel argument: the parameters come from the table, which is what lets a
// captured graph replay the pass.
#include "csg_common.h"
#include "csg_augment.h"
#include "csg_reduce.h"
#include "csg_vec4.h"

namespace csg {

constexpr int kAugThreads = 256;
constexpr int kAugUnroll = 4;
constexpr int kAugMaxGrid = 2048;
static_assert(kAugThreads == CSG_AUG_CHUNK, "a chunk is one pixel per lane of a block");

struct AugParams {
  float b, s, c;
  int tx, ty, y0, x0, size;
};

// shifts beyond +-H move everything out of the map: clamped, so that y - ty cannot overflow
__device__ __forceinline__ AugParams aug_load(const uint32_t* __restrict__ table, int n, int H) {
  const uint4 lo = *(const uint4*)(table + 8 * (size_t)n), hi = *(const uint4*)(table + 8 * (size_t)n + 4);
  AugParams p;
  p.b = __uint_as_float(lo.x);
  p.s = __uint_as_float(lo.y);
  p.c = __uint_as_float(lo.z);
  p.tx = max(-H, min(H, (int)lo.w));
  p.ty = max(-H, min(H, (int)hi.x));
  p.y0 = (int)hi.y;
  p.x0 = (int)hi.z;
  p.size = (int)hi.w;
  return p;
}

__device__ __forceinline__ bool aug_cut(const AugParams& p, int y, int x) {
  return (long long)y >= p.y0 && (long long)y < (long long)p.y0 + p.size && (long long)x >= p.x0 &&
         (long long)x < (long long)p.x0 + p.size;
}

// Forward: out(y, x) <- in(y - ty, x - tx), the cutout tested at (y, x).  Backward: gin(y, x) <- g(y + ty, x + tx), the
// cutout tested at the source.  false: the value is zero.
template <bool BWD>
__device__ __forceinline__ bool aug_source(const AugParams& p, int policy, int H, int y, int x, int& sy, int& sx) {
  sy = y;
  sx = x;
  if (policy & CSG_AUG_TRANSLATION) {
    sy = BWD ? y + p.ty : y - p.ty;
    sx = BWD ? x + p.tx : x - p.tx;
    if ((unsigned)sy >= (unsigned)H || (unsigned)sx >= (unsigned)H) return false;
  }
  if (policy & CSG_AUG_CUTOUT) {
    if (aug_cut(p, BWD ? sy : y, BWD ? sx : x)) return false;
  }
  return true;
}

// the three colour values of the pixel row at px: one 16-byte load, two when the triple straddles two float4
__device__ __forceinline__ void aug_colour3(const float* __restrict__ px, int c0, float& r, float& g, float& b) {
  const int g0 = c0 & ~3;
  const float4 a = ld4(px + g0);
  switch (c0 & 3) {
    case 0: r = a.x; g = a.y; b = a.z; break;
    case 1: r = a.y; g = a.z; b = a.w; break;
    case 2: { const float4 d = ld4(px + g0 + 4); r = a.z; g = a.w; b = d.x; break; }
    default: { const float4 d = ld4(px + g0 + 4); r = a.w; g = d.x; b = d.y; break; }
  }
}

__device__ __forceinline__ void aug_colour_fwd(float& r, float& g, float& b, const AugParams& p, float mu) {
  const float x0 = __fadd_rn(r, p.b), x1 = __fadd_rn(g, p.b), x2 = __fadd_rn(b, p.b);
  const float mp = __fdiv_rn(__fadd_rn(__fadd_rn(x0, x1), x2), 3.0f);
  const float y0 = __fmaf_rn(__fsub_rn(x0, mp), p.s, mp);
  const float y1 = __fmaf_rn(__fsub_rn(x1, mp), p.s, mp);
  const float y2 = __fmaf_rn(__fsub_rn(x2, mp), p.s, mp);
  r = __fmaf_rn(__fsub_rn(y0, mu), p.c, mu);
  g = __fmaf_rn(__fsub_rn(y1, mu), p.c, mu);
  b = __fmaf_rn(__fsub_rn(y2, mu), p.c, mu);
}

__device__ __forceinline__ void aug_colour_bwd(float& r, float& g, float& b, const AugParams& p, float gbar) {
  const float q = __fmul_rn(__fsub_rn(1.0f, p.c), gbar);
  const float a0 = __fmaf_rn(p.c, r, q), a1 = __fmaf_rn(p.c, g, q), a2 = __fmaf_rn(p.c, b, q);
  const float mg = __fdiv_rn(__fadd_rn(__fadd_rn(a0, a1), a2), 3.0f);
  const float w = __fmul_rn(__fsub_rn(1.0f, p.s), mg);
  r = __fmaf_rn(p.s, a0, w);
  g = __fmaf_rn(p.s, a1, w);
  b = __fmaf_rn(p.s, a2, w);
}

// stage 1 of the per-sample sum: one partial per chunk of 256 pixels (forward: of x; backward: of the shifted, masked g)
template <bool BWD>
__global__ __launch_bounds__(kAugThreads) void k_aug_sum(const float* __restrict__ in, const uint32_t* __restrict__ table,
                                                         double* __restrict__ partials, int N, int H, int Ct, int c0, int policy,
                                                         int chunks) {
  __shared__ double part[kAugThreads / 64][1];
  const int total = N * chunks, HH = H * H;
  for (int gc = blockIdx.x; gc < total; gc += gridDim.x) {
    const int n = gc / chunks, pix = (gc - n * chunks) * CSG_AUG_CHUNK + (int)threadIdx.x;
    double v[1] = {0.0};
    if (pix < HH) {
      const int y = pix / H, x = pix - y * H;
      int sy = y, sx = x;
      bool live = true;
      if (BWD) live = aug_source<true>(aug_load(table, n, H), policy, H, y, x, sy, sx);
      if (live) {
        float r, g, b;
        aug_colour3(in + (((size_t)n * H + sy) * H + sx) * Ct, c0, r, g, b);
        v[0] = ((double)r + (double)g) + (double)b;
      }
    }
    block_sum_f64<1, kAugThreads / 64>(v, part);
    if (threadIdx.x == 0) partials[gc] = v[0];
    __syncthreads();                                  // `part` is written again by the next chunk
  }
}

// stage 2: one block per sample adds its partials in a fixed order and rounds the mean once
template <bool BWD>
__global__ __launch_bounds__(kAugThreads) void k_aug_mean(const double* __restrict__ partials, const uint32_t* __restrict__ table,
                                                          float* __restrict__ mean, int chunks, double count) {
  __shared__ double part[kAugThreads / 64][1];
  const int n = blockIdx.x;
  double v[1] = {0.0};
  for (int i = threadIdx.x; i < chunks; i += kAugThreads) v[0] += partials[(size_t)n * chunks + i];
  block_sum_f64<1, kAugThreads / 64>(v, part);
  if (threadIdx.x == 0) {
    double m = v[0] / count;
    if (!BWD) m += (double)__uint_as_float(table[8 * (size_t)n]);       // mu = mean(x) + b
    mean[n] = (float)m;
  }
}

// component j of a float4 at channel 4 * grp + j: colour value ch = 4 * grp + j - c0 if that is 0, 1 or 2
__device__ __forceinline__ float aug_pick(float keep, int ch, float r, float g, float b) {
  return ch == 0 ? r : ch == 1 ? g : ch == 2 ? b : keep;
}

template <bool BWD, bool COLOR>
__global__ __launch_bounds__(kAugThreads) void k_aug_apply(const float* __restrict__ in, float* __restrict__ out,
                                                           const uint32_t* __restrict__ table, const float* __restrict__ mean, int H,
                                                           int Ct, int c0, int policy, unsigned total) {
  const unsigned G = (unsigned)Ct >> 2, HH = (unsigned)(H * H);
  const unsigned base = blockIdx.x * (unsigned)(kAugThreads * kAugUnroll) + threadIdx.x;
  float4 v[kAugUnroll];
  float cr[kAugUnroll], cg[kAugUnroll], cb[kAugUnroll];
  int rel[kAugUnroll];                                // 4 * group - c0 of a lane that holds a colour channel, else INT_MIN
  AugParams prm[kAugUnroll];
  float mu[kAugUnroll];
#pragma unroll
  for (int k = 0; k < kAugUnroll; ++k) {
    const unsigned idx = base + (unsigned)k * kAugThreads;
    v[k] = make_float4(0.f, 0.f, 0.f, 0.f);
    cr[k] = cg[k] = cb[k] = 0.f;
    rel[k] = INT_MIN;
    mu[k] = 0.f;
    if (idx < total) {
      const unsigned q = idx / G, grp = idx - q * G;
      const unsigned n = q / HH, rem = q - n * HH;
      const int y = (int)(rem / (unsigned)H), x = (int)(rem - (unsigned)y * (unsigned)H);
      prm[k] = aug_load(table, (int)n, H);
      int sy, sx;
      const bool live = aug_source<BWD>(prm[k], policy, H, y, x, sy, sx);
      const float* px = in + (((size_t)n * H + sy) * H + sx) * Ct;
      const bool colour = COLOR && (int)(4 * grp) < c0 + 3 && (int)(4 * grp) + 4 > c0;
      if (colour) {
        rel[k] = (int)(4 * grp) - c0;
        mu[k] = mean[n];
      }
      if (live) {
        v[k] = ld4(px + 4 * grp);
        if (colour) aug_colour3(px, c0, cr[k], cg[k], cb[k]);
      } else if (!BWD) {
        rel[k] = INT_MIN;                             // forward: the zero fill comes after the colour map
      }
    }
  }
#pragma unroll
  for (int k = 0; k < kAugUnroll; ++k) {
    const unsigned idx = base + (unsigned)k * kAugThreads;
    if (idx < total) {
      if (COLOR && rel[k] != INT_MIN) {
        if (BWD) aug_colour_bwd(cr[k], cg[k], cb[k], prm[k], mu[k]);
        else aug_colour_fwd(cr[k], cg[k], cb[k], prm[k], mu[k]);
        v[k].x = aug_pick(v[k].x, rel[k], cr[k], cg[k], cb[k]);
        v[k].y = aug_pick(v[k].y, rel[k] + 1, cr[k], cg[k], cb[k]);
        v[k].z = aug_pick(v[k].z, rel[k] + 2, cr[k], cg[k], cb[k]);
        v[k].w = aug_pick(v[k].w, rel[k] + 3, cr[k], cg[k], cb[k]);
      }
      st4(out + 4 * (size_t)idx, v[k]);
    }
  }
}

__global__ __launch_bounds__(kAugThreads) void k_aug_table(uint64_t seed, uint64_t iteration, uint64_t pass, uint64_t rank, int rows,
                                                           int H, uint32_t* __restrict__ table) {
  const int n = blockIdx.x * kAugThreads + threadIdx.x;
  if (n >= rows) return;
  const AugRow r = aug_row(seed, iteration, pass, rank, (uint64_t)n, H);
  *(uint4*)(table + 8 * (size_t)n) = make_uint4(r.w[0], r.w[1], r.w[2], r.w[3]);
  *(uint4*)(table + 8 * (size_t)n + 4) = make_uint4(r.w[4], r.w[5], r.w[6], r.w[7]);
}

static int64_t aug_chunks(int64_t H) { return cdiv(H * H, (int64_t)CSG_AUG_CHUNK); }

static int aug_check_table(const char* who, int64_t iteration, int64_t pass, int64_t rank, int64_t rows, int64_t H) {
  CSG_REQUIRE(iteration >= 0 && pass >= 0 && pass <= 0x7fffffff && rank >= 0 && rank <= 0x7fffffff, CSG_E_BADSHAPE,
              "%s: iteration %ld, pass %ld and rank %ld must be non-negative (pass and rank below 2^31)", who, (long)iteration,
              (long)pass, (long)rank);
  CSG_REQUIRE(rows >= 0 && rows <= 0x7fffffff, CSG_E_BADSHAPE, "%s: %ld rows (0 .. 2^31 - 1)", who, (long)rows);
  CSG_REQUIRE(H >= 2 && H <= CSG_AUG_MAX_H, CSG_E_BADSHAPE, "%s: H = %ld (2 .. %d)", who, (long)H, CSG_AUG_MAX_H);
  return CSG_OK;
}

template <bool BWD>
static int aug_apply(const char* who, const float* in, float* out, const uint32_t* table, int64_t table_rows, int64_t N, int64_t H,
                     int64_t Ct, int64_t c0, int32_t policy, void* workspace, int64_t workspace_bytes, void* stream) {
  CSG_REQUIRE(policy >= 0 && policy <= (CSG_AUG_COLOR | CSG_AUG_TRANSLATION | CSG_AUG_CUTOUT), CSG_E_BADSHAPE,
              "%s: policy %d (a sum of 1 = colour, 2 = translation, 4 = cutout)", who, (int)policy);
  CSG_REQUIRE(H >= 2 && H <= CSG_AUG_MAX_H, CSG_E_BADSHAPE, "%s: H = %ld (2 .. %d)", who, (long)H, CSG_AUG_MAX_H);
  CSG_REQUIRE(Ct >= 4 && Ct % 4 == 0, CSG_E_BADSHAPE, "%s: Ct = %ld must be a positive multiple of 4 (16-byte pixel rows)", who,
              (long)Ct);
  CSG_REQUIRE(c0 >= 0 && c0 + 3 <= Ct, CSG_E_BADSHAPE, "%s: colour channels [%ld, %ld) do not fit Ct = %ld (c0 + 3 > Ct)", who,
              (long)c0, (long)c0 + 3, (long)Ct);
  CSG_REQUIRE(N >= 0 && N <= 0x7fffffff && (double)N * (double)H * (double)H * (double)Ct < 2147483648.0, CSG_E_BADSHAPE,
              "%s: N = %ld samples of %ld x %ld x %ld floats (fewer than 2^31 floats in all)", who, (long)N, (long)H, (long)H,
              (long)Ct);
  CSG_REQUIRE(table_rows >= N, CSG_E_BADSHAPE, "%s: the table has %ld rows, fewer than N = %ld", who, (long)table_rows, (long)N);
  if (N == 0) return CSG_OK;
  CSG_REQUIRE(in != nullptr && out != nullptr && table != nullptr, CSG_E_BADSHAPE, "%s: null pointer", who);
  CSG_REQUIRE((((uintptr_t)in | (uintptr_t)out | (uintptr_t)table) & 15) == 0, CSG_E_BADSHAPE,
              "%s: in, out and the table must be 16-byte aligned", who);
  CSG_REQUIRE((const void*)in != (const void*)out, CSG_E_BADSHAPE, "%s: not in place (a translated pixel reads another one)", who);
  const bool colour = (policy & CSG_AUG_COLOR) != 0;
  const int64_t chunks = aug_chunks(H);
  if (colour)
    CSG_REQUIRE(workspace != nullptr && ((uintptr_t)workspace & 7) == 0 && workspace_bytes >= csg_augment_workspace_bytes(N, H),
                CSG_E_BADSHAPE, "%s: the colour policy needs an 8-byte aligned workspace of %ld bytes (got %ld)", who,
                (long)csg_augment_workspace_bytes(N, H), (long)workspace_bytes);
  hipStream_t s = (hipStream_t)stream;
  double* partials = (double*)workspace;
  float* mean = colour ? (float*)(partials + N * chunks) : nullptr;
  ProfScope p(K_AUGMENT, (double)N * H * H * Ct * 8.0, s);
  if (colour) {
    const int64_t total = N * chunks;
    const unsigned grid = (unsigned)(total < kAugMaxGrid ? total : kAugMaxGrid);
    CSG_LAUNCH(k_aug_sum<BWD>, dim3(grid), dim3(kAugThreads), 0, s, in, table, partials, (int)N, (int)H, (int)Ct, (int)c0,
               (int)policy, (int)chunks);
    CSG_LAUNCH(k_aug_mean<BWD>, dim3((unsigned)N), dim3(kAugThreads), 0, s, (const double*)partials, table, mean, (int)chunks,
               3.0 * (double)H * (double)H);
  }
  const unsigned total4 = (unsigned)(N * H * H * (Ct / 4));
  const unsigned grid = (unsigned)cdiv((int64_t)total4, (int64_t)kAugThreads * kAugUnroll);
  if (colour)
    CSG_LAUNCH((k_aug_apply<BWD, true>), dim3(grid), dim3(kAugThreads), 0, s, in, out, table, (const float*)mean, (int)H, (int)Ct,
               (int)c0, (int)policy, total4);
  else
    CSG_LAUNCH((k_aug_apply<BWD, false>), dim3(grid), dim3(kAugThreads), 0, s, in, out, table, (const float*)mean, (int)H, (int)Ct,
               (int)c0, (int)policy, total4);
  return check_launch(who);
}

}  // namespace csg

using namespace csg;

extern "C" {

int csg_augment_table_host(uint64_t seed, int64_t iteration, int64_t pass, int64_t rank, int64_t rows, int64_t H, uint32_t* table) {
  if (int rc = aug_check_table("csg_augment_table_host", iteration, pass, rank, rows, H)) return rc;
  CSG_REQUIRE(rows == 0 || table != nullptr, CSG_E_BADSHAPE, "csg_augment_table_host: null table");
  for (int64_t n = 0; n < rows; ++n) {
    const AugRow r = aug_row(seed, (uint64_t)iteration, (uint64_t)pass, (uint64_t)rank, (uint64_t)n, (int32_t)H);
    for (int k = 0; k < 8; ++k) table[8 * n + k] = r.w[k];
  }
  return CSG_OK;
}

int csg_augment_table(uint64_t seed, int64_t iteration, int64_t pass, int64_t rank, int64_t rows, int64_t H, uint32_t* table,
                      void* stream) {
  if (int rc = aug_check_table("csg_augment_table", iteration, pass, rank, rows, H)) return rc;
  if (rows == 0) return CSG_OK;
  CSG_REQUIRE(table != nullptr && ((uintptr_t)table & 15) == 0, CSG_E_BADSHAPE, "csg_augment_table: the table must be 16-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  CSG_LAUNCH(k_aug_table, dim3((unsigned)cdiv(rows, (int64_t)kAugThreads)), dim3(kAugThreads), 0, s, seed, (uint64_t)iteration,
             (uint64_t)pass, (uint64_t)rank, (int)rows, (int)H, table);
  return check_launch("csg_augment_table");
}

int64_t csg_augment_workspace_bytes(int64_t N, int64_t H) {
  if (N < 0 || H < 2 || H > CSG_AUG_MAX_H) return -1;
  return (N * aug_chunks(H) * 8 + N * 4 + 15) / 16 * 16;
}

int csg_augment_fwd(const float* in, float* out, const uint32_t* table, int64_t table_rows, int64_t N, int64_t H, int64_t Ct,
                    int64_t c0, int32_t policy, void* workspace, int64_t workspace_bytes, void* stream) {
  return aug_apply<false>("csg_augment_fwd", in, out, table, table_rows, N, H, Ct, c0, policy, workspace, workspace_bytes, stream);
}

int csg_augment_bwd(const float* in, float* out, const uint32_t* table, int64_t table_rows, int64_t N, int64_t H, int64_t Ct,
                    int64_t c0, int32_t policy, void* workspace, int64_t workspace_bytes, void* stream) {
  return aug_apply<true>("csg_augment_bwd", in, out, table, table_rows, N, H, Ct, c0, policy, workspace, workspace_bytes, stream);
}

}  // extern "C"
