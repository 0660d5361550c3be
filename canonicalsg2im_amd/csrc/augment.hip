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
//
// ADAPTIVE STRENGTH (StyleGAN2-ADA; the arithmetic: csg_augment.h).  The _gated entries take one int32 mask per sample beside
// the table: sample n runs policy & gate[n], so "off for this sample" is the same skip as "off for the launch" — bit copies.
// The ungated entries pass a null gate and instantiate the kernels without it: their code is what it was.  k_aug_gate fills
// the masks from the hash and from p24, which it reads from the controller record in device memory; k_ada_accumulate adds
// the signs and the count of the real pass's prediction maps to that record (integer sums, integer atomics: order-free);
// k_ada_update, one thread, moves p24 by one step towards the target and restarts the counts.  None of them takes p as an
// argument or reads anything back, so the gate fills can run eagerly before a replayed step and the accumulation inside it.
#include "csg_common.h"
#include "csg_augment_host.h"
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
// GATED: sample n runs policy & gate[n].  A sample whose colour bit is off needs no mean: its chunks read nothing and write
// 0.0 partials (the block still walks them: the tree and the barriers are per chunk).  Without GATED the code is what it was.
template <bool BWD, bool GATED>
__global__ __launch_bounds__(kAugThreads) void k_aug_sum(const float* __restrict__ in, const uint32_t* __restrict__ table,
                                                         const int32_t* __restrict__ gate, double* __restrict__ partials, int N,
                                                         int H, int Ct, int c0, int policy, int chunks) {
  __shared__ double part[kAugThreads / 64][1];
  const int total = N * chunks, HH = H * H;
  for (int gc = blockIdx.x; gc < total; gc += gridDim.x) {
    const int n = gc / chunks, pix = (gc - n * chunks) * CSG_AUG_CHUNK + (int)threadIdx.x;
    const int pol = GATED ? policy & gate[n] : policy;
    double v[1] = {0.0};
    if (pix < HH && (!GATED || (pol & CSG_AUG_COLOR))) {
      const int y = pix / H, x = pix - y * H;
      int sy = y, sx = x;
      bool live = true;
      if (BWD) live = aug_source<true>(aug_load(table, n, H), pol, H, y, x, sy, sx);
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

// GATED: sample n runs policy & gate[n] — a per-lane value, since a block's float4 may belong to several samples.  A lane of a
// sample whose colour bit is off takes the copy path of a colour-free launch: no second load, no arithmetic on its value.
template <bool BWD, bool COLOR, bool GATED>
__global__ __launch_bounds__(kAugThreads) void k_aug_apply(const float* __restrict__ in, float* __restrict__ out,
                                                           const uint32_t* __restrict__ table, const int32_t* __restrict__ gate,
                                                           const float* __restrict__ mean, int H, int Ct, int c0, int policy,
                                                           unsigned total) {
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
      const int pol = GATED ? policy & gate[n] : policy;
      int sy, sx;
      const bool live = aug_source<BWD>(prm[k], pol, H, y, x, sy, sx);
      const float* px = in + (((size_t)n * H + sy) * H + sx) * Ct;
      const bool colour = COLOR && (!GATED || (pol & CSG_AUG_COLOR)) && (int)(4 * grp) < c0 + 3 && (int)(4 * grp) + 4 > c0;
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

__global__ __launch_bounds__(kAugThreads) void k_aug_gate(uint64_t seed, uint64_t iteration, uint64_t pass, uint64_t rank, int rows,
                                                          const int64_t* __restrict__ ctrl, int32_t* __restrict__ gate) {
  const int n = blockIdx.x * kAugThreads + threadIdx.x;
  if (n >= rows) return;
  gate[n] = (int32_t)aug_gate(seed, iteration, pass, rank, (uint64_t)n, (uint32_t)ada_clamp_p(ctrl[0]));
}

// The overfitting figure of StyleGAN2-ADA, r_t = E[sign(D(real))], as two integers: S += sum of sign(x), C += the number of
// elements, over every element of up to four prediction maps (the item form of csg_hinge_mean_fwd).  sign: +1 for x > 0, -1
// for x < 0, else 0 (both zeros, NaN).  Integer sums do not depend on their order: a lane strides over the flat element
// index, a block adds its lanes (shuffles, then the four waves), and lane 0 adds the block's pair to the record with two
// 64-bit integer atomics — the same words whatever the grid.
constexpr int kAdaMaxGrid = 256;

struct AdaItems {
  const float* x[4];
  int64_t sb[4], sh[4], sw[4];
  int64_t first[5];               // map m holds elements [first[m], first[m + 1]) of the launch; an absent map none
  int H[4], W[4];
  int n;
};

__global__ __launch_bounds__(kAugThreads) void k_ada_accumulate(AdaItems it, int64_t* __restrict__ ctrl) {
  __shared__ long long part[kAugThreads / 64][2];
  long long sum = 0, cnt = 0;
#pragma unroll
  for (int m = 0; m < 4; ++m) {                       // (constant indices: the items stay in the kernel's arguments)
    const int64_t count = it.first[m + 1] - it.first[m], hw = (int64_t)it.H[m] * it.W[m];
    for (int64_t e = (int64_t)blockIdx.x * kAugThreads + threadIdx.x; e < count; e += (int64_t)gridDim.x * kAugThreads) {
      const int64_t b = e / hw, r = e - b * hw;
      const int64_t y = r / it.W[m], x = r - y * it.W[m];
      const float v = it.x[m][b * it.sb[m] + y * it.sh[m] + x * it.sw[m]];
      sum += (v > 0.0f) ? 1 : (v < 0.0f) ? -1 : 0;
      cnt += 1;
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    sum += __shfl_down(sum, o, 64);
    cnt += __shfl_down(cnt, o, 64);
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) {
    part[wave][0] = sum;
    part[wave][1] = cnt;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    long long S = 0, C = 0;
    for (int w = 0; w < kAugThreads / 64; ++w) {
      S += part[w][0];
      C += part[w][1];
    }
    if (C) {
      atomicAdd((unsigned long long*)(ctrl + 1), (unsigned long long)S);
      atomicAdd((unsigned long long*)(ctrl + 2), (unsigned long long)C);
    }
  }
}

__global__ void k_ada_update(int64_t* __restrict__ ctrl, int64_t T24, int64_t step24) {
  if (blockIdx.x == 0 && threadIdx.x == 0) ada_update_words(ctrl, T24, step24);
}

static int64_t aug_chunks(int64_t H) { return cdiv(H * H, (int64_t)CSG_AUG_CHUNK); }

static int aug_check_table(const char* who, int64_t iteration, int64_t pass, int64_t rank, int64_t rows, int64_t H) {
  if (int rc = aug_check_key(who, iteration, pass, rank, rows, 0x7fffffff, "0 .. 2^31 - 1")) return rc;
  return aug_check_h(who, H);
}

template <bool BWD>
static int aug_apply(const char* who, const float* in, float* out, const uint32_t* table, int64_t table_rows, int64_t N, int64_t H,
                     int64_t Ct, int64_t c0, int32_t policy, void* workspace, int64_t workspace_bytes, bool gated,
                     const int32_t* gate, void* stream) {
  CSG_REQUIRE(policy >= 0 && policy <= (CSG_AUG_COLOR | CSG_AUG_TRANSLATION | CSG_AUG_CUTOUT), CSG_E_BADSHAPE,
              "%s: policy %d (a sum of 1 = colour, 2 = translation, 4 = cutout)", who, (int)policy);
  bool empty;
  if (int rc = aug_check_map(who, in, out, table, table_rows, N, H, Ct, c0, "a translated pixel reads another one", empty)) return rc;
  if (empty) return CSG_OK;
  if (gated)
    CSG_REQUIRE(gate != nullptr && ((uintptr_t)gate & 3) == 0, CSG_E_BADSHAPE,
                "%s: the gate must be a 4-byte aligned array of N int32 (null pointer or misaligned)", who);
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
    if (gated)
      CSG_LAUNCH((k_aug_sum<BWD, true>), dim3(grid), dim3(kAugThreads), 0, s, in, table, gate, partials, (int)N, (int)H, (int)Ct,
                 (int)c0, (int)policy, (int)chunks);
    else
      CSG_LAUNCH((k_aug_sum<BWD, false>), dim3(grid), dim3(kAugThreads), 0, s, in, table, gate, partials, (int)N, (int)H, (int)Ct,
                 (int)c0, (int)policy, (int)chunks);
    CSG_LAUNCH(k_aug_mean<BWD>, dim3((unsigned)N), dim3(kAugThreads), 0, s, (const double*)partials, table, mean, (int)chunks,
               3.0 * (double)H * (double)H);
  }
  const unsigned total4 = (unsigned)(N * H * H * (Ct / 4));
  const unsigned grid = (unsigned)cdiv((int64_t)total4, (int64_t)kAugThreads * kAugUnroll);
#define CSG_AUG_APPLY(COLOR, GATED)                                                                                          \
  CSG_LAUNCH((k_aug_apply<BWD, COLOR, GATED>), dim3(grid), dim3(kAugThreads), 0, s, in, out, table, gate, (const float*)mean, \
             (int)H, (int)Ct, (int)c0, (int)policy, total4)
  if (colour && gated) CSG_AUG_APPLY(true, true);
  else if (colour) CSG_AUG_APPLY(true, false);
  else if (gated) CSG_AUG_APPLY(false, true);
  else CSG_AUG_APPLY(false, false);
#undef CSG_AUG_APPLY
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
  return aug_apply<false>("csg_augment_fwd", in, out, table, table_rows, N, H, Ct, c0, policy, workspace, workspace_bytes, false,
                          nullptr, stream);
}

int csg_augment_bwd(const float* in, float* out, const uint32_t* table, int64_t table_rows, int64_t N, int64_t H, int64_t Ct,
                    int64_t c0, int32_t policy, void* workspace, int64_t workspace_bytes, void* stream) {
  return aug_apply<true>("csg_augment_bwd", in, out, table, table_rows, N, H, Ct, c0, policy, workspace, workspace_bytes, false,
                         nullptr, stream);
}

int csg_augment_fwd_gated(const float* in, float* out, const uint32_t* table, int64_t table_rows, int64_t N, int64_t H, int64_t Ct,
                          int64_t c0, int32_t policy, void* workspace, int64_t workspace_bytes, const int32_t* gate, void* stream) {
  return aug_apply<false>("csg_augment_fwd_gated", in, out, table, table_rows, N, H, Ct, c0, policy, workspace, workspace_bytes,
                          true, gate, stream);
}

int csg_augment_bwd_gated(const float* in, float* out, const uint32_t* table, int64_t table_rows, int64_t N, int64_t H, int64_t Ct,
                          int64_t c0, int32_t policy, void* workspace, int64_t workspace_bytes, const int32_t* gate, void* stream) {
  return aug_apply<true>("csg_augment_bwd_gated", in, out, table, table_rows, N, H, Ct, c0, policy, workspace, workspace_bytes,
                         true, gate, stream);
}

int csg_augment_gate_host(uint64_t seed, int64_t iteration, int64_t pass, int64_t rank, int64_t rows, int64_t p24, int32_t* gate) {
  if (int rc = aug_check_key("csg_augment_gate_host", iteration, pass, rank, rows, 0x7fffffff, "0 .. 2^31 - 1")) return rc;
  if (int rc = aug_check_p24("csg_augment_gate_host", p24)) return rc;
  CSG_REQUIRE(rows == 0 || gate != nullptr, CSG_E_BADSHAPE, "csg_augment_gate_host: null pointer");
  for (int64_t n = 0; n < rows; ++n)
    gate[n] = (int32_t)aug_gate(seed, (uint64_t)iteration, (uint64_t)pass, (uint64_t)rank, (uint64_t)n, (uint32_t)p24);
  return CSG_OK;
}

int csg_augment_gate(uint64_t seed, int64_t iteration, int64_t pass, int64_t rank, int64_t rows, const int64_t* ctrl, int32_t* gate,
                     void* stream) {
  if (int rc = aug_check_key("csg_augment_gate", iteration, pass, rank, rows, 0x7fffffff, "0 .. 2^31 - 1")) return rc;
  if (int rc = aug_check_ctrl("csg_augment_gate", ctrl)) return rc;
  if (rows == 0) return CSG_OK;
  CSG_REQUIRE(gate != nullptr && ((uintptr_t)gate & 3) == 0, CSG_E_BADSHAPE,
              "csg_augment_gate: the gate must be 4-byte aligned (null pointer or misaligned)");
  hipStream_t s = (hipStream_t)stream;
  CSG_LAUNCH(k_aug_gate, dim3((unsigned)cdiv(rows, (int64_t)kAugThreads)), dim3(kAugThreads), 0, s, seed, (uint64_t)iteration,
             (uint64_t)pass, (uint64_t)rank, (int)rows, ctrl, gate);
  return check_launch("csg_augment_gate");
}

int csg_ada_accumulate(const csg_hinge_item* items, int32_t n_items, int64_t* ctrl, void* stream) {
  CSG_REQUIRE(items != nullptr && n_items >= 1 && n_items <= 4, CSG_E_BADSHAPE, "csg_ada_accumulate: 1..4 maps (got %d)",
              (int)n_items);
  if (int rc = aug_check_ctrl("csg_ada_accumulate", ctrl)) return rc;
  AdaItems it;
  it.n = n_items;
  int64_t total = 0;
  for (int i = 0; i < 4; ++i) {
    const csg_hinge_item& d = items[i < n_items ? i : 0];
    CSG_REQUIRE(d.x != nullptr && ((uintptr_t)d.x & 3) == 0 && d.B > 0 && d.H > 0 && d.W > 0 && d.B * d.H * d.W < (1ll << 30),
                CSG_E_BADSHAPE, "csg_ada_accumulate: bad map %d (null pointer, misaligned, or not 1 .. 2^30 - 1 elements)", i);
    it.x[i] = d.x; it.sb[i] = d.sb; it.sh[i] = d.sh; it.sw[i] = d.sw;
    it.H[i] = (int)d.H; it.W[i] = (int)d.W;
    it.first[i] = total;
    if (i < n_items) total += d.B * d.H * d.W;
  }
  it.first[4] = total;
  hipStream_t s = (hipStream_t)stream;
  const int64_t blocks = cdiv(total, (int64_t)kAugThreads * 4);
  ProfScope p(K_AUGMENT, (double)total * 4.0, s);
  CSG_LAUNCH(k_ada_accumulate, dim3((unsigned)(blocks < kAdaMaxGrid ? blocks : kAdaMaxGrid)), dim3(kAugThreads), 0, s, it, ctrl);
  return check_launch("csg_ada_accumulate");
}

static int ada_check_update(const char* who, const int64_t* ctrl, int64_t T24, int64_t step24) {
  if (int rc = aug_check_ctrl(who, ctrl)) return rc;
  CSG_REQUIRE(T24 >= 0 && T24 <= CSG_ADA_ONE, CSG_E_BADSHAPE, "%s: T24 = %ld (0 .. 2^24)", who, (long)T24);
  CSG_REQUIRE(step24 >= 1, CSG_E_BADSHAPE, "%s: step24 = %ld (step24 < 1)", who, (long)step24);
  return CSG_OK;
}

int csg_ada_update_host(int64_t* ctrl, int64_t T24, int64_t step24) {
  if (int rc = ada_check_update("csg_ada_update_host", ctrl, T24, step24)) return rc;
  if (int rc = aug_check_p24("csg_ada_update_host", ctrl[0])) return rc;
  CSG_REQUIRE(ctrl[2] >= 0 && ctrl[2] < CSG_ADA_MAX_COUNT, CSG_E_BADSHAPE,
              "csg_ada_update_host: C = %ld elements (0 .. 2^38 - 1: S * 2^24 must fit int64)", (long)ctrl[2]);
  ada_update_words(ctrl, T24, step24);
  return CSG_OK;
}

// The device twin cannot read the words before the launch: a p24 outside [0, 2^24] is clamped and a count outside
// [0, 2^38) leaves p24 alone (csg_augment.h), where the host entry refuses.
int csg_ada_update(int64_t* ctrl, int64_t T24, int64_t step24, void* stream) {
  if (int rc = ada_check_update("csg_ada_update", ctrl, T24, step24)) return rc;
  hipStream_t s = (hipStream_t)stream;
  CSG_LAUNCH(k_ada_update, dim3(1), dim3(1), 0, s, ctrl, T24, step24);
  return check_launch("csg_ada_update");
}

}  // extern "C"
