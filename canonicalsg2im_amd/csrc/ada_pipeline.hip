// The ADA augmentation pipeline (StyleGAN2-ADA, Karras et al., NeurIPS 2020, appendix B) of what the discriminators see:
// pixel blitting, general geometry and linear colour transforms of an NHWC map with a padded channel count, as ONE per-sample
// affine resampling followed by a 3 x 4 colour matrix; forward, exact adjoint, and the parameter table both read
// (include/csg_hip.h, "The ADA augmentation pipeline"; the row, the draws and the fp64 composition: csg_ada_pipeline.h).
//
// DEVIATIONS from the authors' pipeline, on purpose: four bilinear taps instead of the wavelet up / down-sampling around the
// resampler, zero fill instead of reflection padding (as DiffAugment's translation here), a bounded "normal" and clamped
// scales (csg_ada_pipeline.h).
//
// THE fp32 OPERATION SEQUENCE (the contract tests/ada_pipeline_cases.py restates; compiled with -ffp-contract=off, every
// multiplication and addition separate).  One sample x of shape (H, H, Ct), its row (M, G, margin, flags, C, integer map),
// c = (H - 1) / 2 (exact in fp32: H <= 16384).  Forward, per output pixel (x, y):
//     x' = (float)x - c;  y' = (float)y - c                                exact
//     sx = (m00 * x' + m01 * y') + m02;  sy = (m10 * x' + m11 * y') + m12
//     a coordinate that is not |s| < 2^23 (a NaN fails the comparison) gives no taps and is never converted to an integer
//     x0 = floor(sx);  fx = sx - x0 (exact);  wx0 = 1 - fx (one rounding);  wx1 = fx;  y likewise
//     taps a00 = in(y0, x0), a01 = in(y0, x0 + 1), a10 = in(y0 + 1, x0), a11 = in(y0 + 1, x0 + 1); a tap outside [0, H)^2 is
//     0 and is not loaded;  w00 = wy0 * wx0, w01 = wy0 * wx1, w10 = wy1 * wx0, w11 = wy1 * wx1
//     v = ((w00 * a00 + w01 * a01) + w10 * a10) + w11 * a11               4 products, 3 additions: ADA_INTERP_ROUNDINGS = 7
//     colour channels, from the interpolated (r, g, b):  r' = ((c00 * r + c01 * g) + c02 * b) + c03, g', b' likewise
//                                                                          3 products, 3 additions: ADA_COLOR_ROUNDINGS = 6
// The matrix acts on the interpolated value, so a zero-filled pixel takes the brightness offset.  Paths by flag:
// CSG_ADA_GEOM_ID copies the source pixel; CSG_ADA_GEOM_INT copies in(sy, sx), sx = a x + b y + ex, sy = c x + d y + ey, zero
// outside (ex, ey are clamped to +-2^20 — beyond +-2 H everything is outside —, and a row whose (a b; c d) is not a signed
// permutation gives zeros); CSG_ADA_COLOR_ID runs no arithmetic on the colour channels.  All three: a bit copy.
//
// BACKWARD, the exact adjoint in gather form, no atomics.  For a source pixel q = (qx, qy):
//     q' = q - c;  cx = (g00 * qx' + g01 * qy') + g02;  hx = |g00| + |g01|;  cy, hy likewise;  m = clamp(margin, 0, 4)
//     the box  x in [floor(cx - hx) - m, ceil(cx + hx) + m], y likewise, clamped to the map and then to CSG_ADA_MAX_BOX a side
//     (a centre that is not |cx| + hx < 2^23 gives an empty box), walked in ROW-MAJOR order; per output pixel p the forward's
//     sx, sy, x0, fx, y0, fy by the forward's sequence — the same bits —; where qx - x0 is 0 or 1 and qy - y0 is 0 or 1:
//         w = wy * wx  (the forward's weight of that tap);   acc = acc + w * t(p)           ADA_ADJOINT_TERM_ROUNDINGS = 1 + 1
//     t(p) = g(p) on the other channels and with CSG_ADA_COLOR_ID;  on the colour channels
//         t_j = (c0j * g_0 + c1j * g_1) + c2j * g_2                         3 products, 2 additions
// The order of the sum is fixed by q alone: the same bits on every run and for every grid.  The copy paths copy: with
// CSG_ADA_GEOM_ID gin(q) = t(q), with CSG_ADA_GEOM_INT gin(q) = t(P^T (q - e)) or zero.  A generated row's box holds every
// output pixel that has q among its taps (csg_ada_pipeline.h, THE SEARCH BOX); for a caller's row whose G is not M's inverse or
// is larger than that the walk is what is stated here, no more.
//
// ACCESS.  One lane owns one float4 of a pixel (csg_vec4.h); a tap is a contiguous Ct * 4-byte row that consecutive lanes read
// together; every load of a lane is issued before its one store.  A lane whose float4 holds a colour channel fetches the
// pixel's other colour float4 again when the triple straddles two (it hits L1 / L2).  Nothing that varies per step is a
// kernel argument: the parameters come from the table, which is what lets a captured graph replay the pass.
#include "csg_common.h"
#include "csg_ada_pipeline.h"
#include "csg_augment_host.h"
#include "csg_vec4.h"

namespace csg {

constexpr int kAdaThreads = 256;

struct AdaGeo {
  float m[6], g[6];
  uint32_t flags;
  int margin, ex, ey, a, b, c, d;
};

__device__ __forceinline__ AdaGeo ada_load_geo(const uint32_t* __restrict__ row) {
  const uint4 w0 = *(const uint4*)row, w1 = *(const uint4*)(row + 4), w2 = *(const uint4*)(row + 8);
  const uint4 mf = *(const uint4*)(row + 12), pm = *(const uint4*)(row + 28);
  AdaGeo g;
  g.m[0] = __uint_as_float(w0.x); g.m[1] = __uint_as_float(w0.y); g.m[2] = __uint_as_float(w0.z);
  g.m[3] = __uint_as_float(w0.w); g.m[4] = __uint_as_float(w1.x); g.m[5] = __uint_as_float(w1.y);
  g.g[0] = __uint_as_float(w1.z); g.g[1] = __uint_as_float(w1.w); g.g[2] = __uint_as_float(w2.x);
  g.g[3] = __uint_as_float(w2.y); g.g[4] = __uint_as_float(w2.z); g.g[5] = __uint_as_float(w2.w);
  g.margin = max(0, min(CSG_ADA_MAX_MARGIN, (int)mf.x));
  g.flags = mf.y;
  g.ex = max(-(1 << 20), min(1 << 20, (int)mf.z));
  g.ey = max(-(1 << 20), min(1 << 20, (int)mf.w));
  g.a = (int)pm.x; g.b = (int)pm.y; g.c = (int)pm.z; g.d = (int)pm.w;
  return g;
}

__device__ __forceinline__ bool ada_signed_perm(const AdaGeo& g) {
  const bool unit = (g.a == 0 || g.a == 1 || g.a == -1) && (g.b == 0 || g.b == 1 || g.b == -1) &&
                    (g.c == 0 || g.c == 1 || g.c == -1) && (g.d == 0 || g.d == 1 || g.d == -1);
  return unit && abs(g.a) + abs(g.b) == 1 && abs(g.c) + abs(g.d) == 1 && abs(g.a) + abs(g.c) == 1;
}

struct AdaCMat {
  float c[12];
};

__device__ __forceinline__ AdaCMat ada_load_colour(const uint32_t* __restrict__ row) {
  const uint4 r0 = *(const uint4*)(row + 16), r1 = *(const uint4*)(row + 20), r2 = *(const uint4*)(row + 24);
  AdaCMat C;
  C.c[0] = __uint_as_float(r0.x); C.c[1] = __uint_as_float(r0.y); C.c[2] = __uint_as_float(r0.z); C.c[3] = __uint_as_float(r0.w);
  C.c[4] = __uint_as_float(r1.x); C.c[5] = __uint_as_float(r1.y); C.c[6] = __uint_as_float(r1.z); C.c[7] = __uint_as_float(r1.w);
  C.c[8] = __uint_as_float(r2.x); C.c[9] = __uint_as_float(r2.y); C.c[10] = __uint_as_float(r2.z); C.c[11] = __uint_as_float(r2.w);
  return C;
}

// one axis of the forward's coordinate: false when s is not |s| < 2^23
__device__ __forceinline__ bool ada_axis(float s, int& i0, float& w0, float& w1) {
  if (!(fabsf(s) < 8388608.0f)) return false;
  const float f0 = floorf(s);
  w1 = __fsub_rn(s, f0);
  w0 = __fsub_rn(1.0f, w1);
  i0 = (int)f0;
  return true;
}

__device__ __forceinline__ void ada_coord(const float* m, float xc, float yc, float& sx, float& sy) {
  sx = __fadd_rn(__fadd_rn(__fmul_rn(m[0], xc), __fmul_rn(m[1], yc)), m[2]);
  sy = __fadd_rn(__fadd_rn(__fmul_rn(m[3], xc), __fmul_rn(m[4], yc)), m[5]);
}

// what one output pixel reads: a copy of one pixel, nothing, or four weighted taps (offsets in floats; -1: not loaded)
struct AdaTaps {
  int mode;                                         // 0 copy of o[0], 1 zero, 2 bilinear
  long long o[4];
  float w[4];
};

__device__ __forceinline__ float4 ada_sample(const float* __restrict__ in, const AdaTaps& t, int grp) {
  const float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
  if (t.mode == 0) return ld4(in + t.o[0] + 4 * grp);
  if (t.mode == 1) return z;
  const float4 a0 = t.o[0] >= 0 ? ld4(in + t.o[0] + 4 * grp) : z, a1 = t.o[1] >= 0 ? ld4(in + t.o[1] + 4 * grp) : z;
  const float4 a2 = t.o[2] >= 0 ? ld4(in + t.o[2] + 4 * grp) : z, a3 = t.o[3] >= 0 ? ld4(in + t.o[3] + 4 * grp) : z;
  float4 v;
#define CSG_ADA_MIX(f)                                                                                                       \
  v.f = __fadd_rn(__fadd_rn(__fadd_rn(__fmul_rn(t.w[0], a0.f), __fmul_rn(t.w[1], a1.f)), __fmul_rn(t.w[2], a2.f)), \
                  __fmul_rn(t.w[3], a3.f))
  CSG_ADA_MIX(x);
  CSG_ADA_MIX(y);
  CSG_ADA_MIX(z);
  CSG_ADA_MIX(w);
#undef CSG_ADA_MIX
  return v;
}

// component j of the float4 of group grp: colour value k = 4 * grp + j - c0 if that is 0, 1 or 2
__device__ __forceinline__ float ada_pick(float keep, int k, float r, float g, float b) {
  return k == 0 ? r : k == 1 ? g : k == 2 ? b : keep;
}

// the colour triple out of the float4s of groups c0 / 4 (lo) and c0 / 4 + 1 (hi; unused unless the triple straddles)
__device__ __forceinline__ void ada_triple(const float4& lo, const float4& hi, int c0, float& r, float& g, float& b) {
  switch (c0 & 3) {
    case 0: r = lo.x; g = lo.y; b = lo.z; break;
    case 1: r = lo.y; g = lo.z; b = lo.w; break;
    case 2: r = lo.z; g = lo.w; b = hi.x; break;
    default: r = lo.w; g = hi.x; b = hi.y; break;
  }
}

__device__ __forceinline__ bool ada_colour_lane(int grp, int c0) { return 4 * grp < c0 + 3 && 4 * grp + 4 > c0; }

__global__ __launch_bounds__(kAdaThreads) void k_ada_pipeline_fwd(const float* __restrict__ in, float* __restrict__ out,
                                                                  const uint32_t* __restrict__ table, int H, int Ct, int c0,
                                                                  unsigned total) {
  const unsigned idx = blockIdx.x * (unsigned)kAdaThreads + threadIdx.x;
  if (idx >= total) return;
  const unsigned G = (unsigned)Ct >> 2, HH = (unsigned)(H * H);
  const unsigned q = idx / G;
  const int grp = (int)(idx - q * G);
  const unsigned n = q / HH, rem = q - n * HH;
  const int y = (int)(rem / (unsigned)H), x = (int)(rem - (unsigned)y * (unsigned)H);
  const uint32_t* row = table + (size_t)CSG_ADA_ROW_WORDS * n;
  const AdaGeo geo = ada_load_geo(row);
  const long long base = (long long)n * HH * Ct;
  AdaTaps t;
  t.mode = 1;
  t.o[0] = t.o[1] = t.o[2] = t.o[3] = -1;
  t.w[0] = t.w[1] = t.w[2] = t.w[3] = 0.f;
  if (geo.flags & CSG_ADA_GEOM_ID) {
    t.mode = 0;
    t.o[0] = base + ((long long)y * H + x) * Ct;
  } else if (geo.flags & CSG_ADA_GEOM_INT) {
    const long long sx = (long long)geo.a * x + (long long)geo.b * y + geo.ex, sy = (long long)geo.c * x + (long long)geo.d * y + geo.ey;
    if (ada_signed_perm(geo) && sx >= 0 && sx < H && sy >= 0 && sy < H) {
      t.mode = 0;
      t.o[0] = base + (sy * H + sx) * Ct;
    }
  } else {
    const float c = (float)(H - 1) * 0.5f;
    float sx, sy, wx0, wx1, wy0, wy1;
    int x0, y0;
    ada_coord(geo.m, (float)x - c, (float)y - c, sx, sy);
    if (ada_axis(sx, x0, wx0, wx1) && ada_axis(sy, y0, wy0, wy1)) {
      t.mode = 2;
      const bool lx0 = (unsigned)x0 < (unsigned)H, lx1 = (unsigned)(x0 + 1) < (unsigned)H;
      const bool ly0 = (unsigned)y0 < (unsigned)H, ly1 = (unsigned)(y0 + 1) < (unsigned)H;
      const long long p = base + ((long long)y0 * H + x0) * Ct;
      t.o[0] = ly0 && lx0 ? p : -1;
      t.o[1] = ly0 && lx1 ? p + Ct : -1;
      t.o[2] = ly1 && lx0 ? p + (long long)H * Ct : -1;
      t.o[3] = ly1 && lx1 ? p + (long long)H * Ct + Ct : -1;
      t.w[0] = __fmul_rn(wy0, wx0);
      t.w[1] = __fmul_rn(wy0, wx1);
      t.w[2] = __fmul_rn(wy1, wx0);
      t.w[3] = __fmul_rn(wy1, wx1);
    }
  }
  float4 v = ada_sample(in, t, grp);
  if (!(geo.flags & CSG_ADA_COLOR_ID) && ada_colour_lane(grp, c0)) {
    const int g0 = c0 >> 2;
    const bool straddle = (c0 & 3) >= 2;
    const float4 lo = grp == g0 ? v : ada_sample(in, t, g0);
    const float4 hi = !straddle ? lo : grp == g0 + 1 ? v : ada_sample(in, t, g0 + 1);
    float r, g, b;
    ada_triple(lo, hi, c0, r, g, b);
    const AdaCMat C = ada_load_colour(row);
    const float r2 = __fadd_rn(__fadd_rn(__fadd_rn(__fmul_rn(C.c[0], r), __fmul_rn(C.c[1], g)), __fmul_rn(C.c[2], b)), C.c[3]);
    const float g2 = __fadd_rn(__fadd_rn(__fadd_rn(__fmul_rn(C.c[4], r), __fmul_rn(C.c[5], g)), __fmul_rn(C.c[6], b)), C.c[7]);
    const float b2 = __fadd_rn(__fadd_rn(__fadd_rn(__fmul_rn(C.c[8], r), __fmul_rn(C.c[9], g)), __fmul_rn(C.c[10], b)), C.c[11]);
    const int k = 4 * grp - c0;
    v.x = ada_pick(v.x, k, r2, g2, b2);
    v.y = ada_pick(v.y, k + 1, r2, g2, b2);
    v.z = ada_pick(v.z, k + 2, r2, g2, b2);
    v.w = ada_pick(v.w, k + 3, r2, g2, b2);
  }
  st4(out + 4 * (size_t)idx, v);
}

// t(p) of the header: the gradient at output pixel p (offset o, in floats) as this lane's float4 of the source sees it
__device__ __forceinline__ float4 ada_grad_at(const float* __restrict__ g, long long o, int grp, int c0, bool colour,
                                              const AdaCMat& C) {
  float4 v = ld4(g + o + 4 * grp);
  if (colour) {
    const int g0 = c0 >> 2;
    const bool straddle = (c0 & 3) >= 2;
    const float4 lo = grp == g0 ? v : ld4(g + o + 4 * g0);
    const float4 hi = !straddle ? lo : grp == g0 + 1 ? v : ld4(g + o + 4 * (g0 + 1));
    float a, b, c;
    ada_triple(lo, hi, c0, a, b, c);
    const float t0 = __fadd_rn(__fadd_rn(__fmul_rn(C.c[0], a), __fmul_rn(C.c[4], b)), __fmul_rn(C.c[8], c));
    const float t1 = __fadd_rn(__fadd_rn(__fmul_rn(C.c[1], a), __fmul_rn(C.c[5], b)), __fmul_rn(C.c[9], c));
    const float t2 = __fadd_rn(__fadd_rn(__fmul_rn(C.c[2], a), __fmul_rn(C.c[6], b)), __fmul_rn(C.c[10], c));
    const int k = 4 * grp - c0;
    v.x = ada_pick(v.x, k, t0, t1, t2);
    v.y = ada_pick(v.y, k + 1, t0, t1, t2);
    v.z = ada_pick(v.z, k + 2, t0, t1, t2);
    v.w = ada_pick(v.w, k + 3, t0, t1, t2);
  }
  return v;
}

__global__ __launch_bounds__(kAdaThreads) void k_ada_pipeline_bwd(const float* __restrict__ g, float* __restrict__ gin,
                                                                  const uint32_t* __restrict__ table, int H, int Ct, int c0,
                                                                  unsigned total) {
  const unsigned idx = blockIdx.x * (unsigned)kAdaThreads + threadIdx.x;
  if (idx >= total) return;
  const unsigned G = (unsigned)Ct >> 2, HH = (unsigned)(H * H);
  const unsigned q = idx / G;
  const int grp = (int)(idx - q * G);
  const unsigned n = q / HH, rem = q - n * HH;
  const int qy = (int)(rem / (unsigned)H), qx = (int)(rem - (unsigned)qy * (unsigned)H);
  const uint32_t* row = table + (size_t)CSG_ADA_ROW_WORDS * n;
  const AdaGeo geo = ada_load_geo(row);
  const long long base = (long long)n * HH * Ct;
  const bool colour = !(geo.flags & CSG_ADA_COLOR_ID) && ada_colour_lane(grp, c0);
  AdaCMat C;
#pragma unroll
  for (int i = 0; i < 12; ++i) C.c[i] = 0.f;
  if (colour) C = ada_load_colour(row);
  float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
  if (geo.flags & CSG_ADA_GEOM_ID) {
    acc = ada_grad_at(g, base + ((long long)qy * H + qx) * Ct, grp, c0, colour, C);
  } else if (geo.flags & CSG_ADA_GEOM_INT) {
    // the inverse of a signed permutation is its transpose
    const long long ux = (long long)qx - geo.ex, uy = (long long)qy - geo.ey;
    const long long px = geo.a * ux + geo.c * uy, py = geo.b * ux + geo.d * uy;
    if (ada_signed_perm(geo) && px >= 0 && px < H && py >= 0 && py < H)
      acc = ada_grad_at(g, base + (py * H + px) * Ct, grp, c0, colour, C);
  } else {
    const float c = (float)(H - 1) * 0.5f;
    float cx, cy;
    ada_coord(geo.g, (float)qx - c, (float)qy - c, cx, cy);
    const float hx = __fadd_rn(fabsf(geo.g[0]), fabsf(geo.g[1])), hy = __fadd_rn(fabsf(geo.g[3]), fabsf(geo.g[4]));
    if (__fadd_rn(fabsf(cx), hx) < 8388608.0f && __fadd_rn(fabsf(cy), hy) < 8388608.0f) {
      int xlo = max((int)floorf(__fsub_rn(cx, hx)) - geo.margin, 0), xhi = min((int)ceilf(__fadd_rn(cx, hx)) + geo.margin, H - 1);
      int ylo = max((int)floorf(__fsub_rn(cy, hy)) - geo.margin, 0), yhi = min((int)ceilf(__fadd_rn(cy, hy)) + geo.margin, H - 1);
      xhi = min(xhi, xlo + CSG_ADA_MAX_BOX - 1);
      yhi = min(yhi, ylo + CSG_ADA_MAX_BOX - 1);
      for (int py = ylo; py <= yhi; ++py) {
        for (int px = xlo; px <= xhi; ++px) {
          float sx, sy, wx0, wx1, wy0, wy1;
          int x0, y0;
          ada_coord(geo.m, (float)px - c, (float)py - c, sx, sy);
          if (!(ada_axis(sx, x0, wx0, wx1) && ada_axis(sy, y0, wy0, wy1))) continue;
          const int dx = qx - x0, dy = qy - y0;
          if ((unsigned)dx > 1u || (unsigned)dy > 1u) continue;
          const float w = __fmul_rn(dy ? wy1 : wy0, dx ? wx1 : wx0);
          const float4 t = ada_grad_at(g, base + ((long long)py * H + px) * Ct, grp, c0, colour, C);
          acc.x = __fadd_rn(acc.x, __fmul_rn(w, t.x));
          acc.y = __fadd_rn(acc.y, __fmul_rn(w, t.y));
          acc.z = __fadd_rn(acc.z, __fmul_rn(w, t.z));
          acc.w = __fadd_rn(acc.w, __fmul_rn(w, t.w));
        }
      }
    }
  }
  st4(gin + 4 * (size_t)idx, acc);
}

__global__ __launch_bounds__(kAdaThreads) void k_ada_pipeline_table(uint64_t seed, uint64_t iteration, uint64_t pass, uint64_t rank,
                                                                    int rows, int H, int policy, const int64_t* __restrict__ ctrl,
                                                                    uint32_t* __restrict__ table) {
  const int n = blockIdx.x * kAdaThreads + threadIdx.x;
  if (n >= rows) return;
  const AdaRow r = ada_row(seed, iteration, pass, rank, (uint64_t)n, H, policy, (uint32_t)ada_clamp_p(ctrl[0]));
  uint4* dst = (uint4*)(table + (size_t)CSG_ADA_ROW_WORDS * n);
#pragma unroll
  for (int k = 0; k < CSG_ADA_ROW_WORDS / 4; ++k) dst[k] = make_uint4(r.w[4 * k], r.w[4 * k + 1], r.w[4 * k + 2], r.w[4 * k + 3]);
}

static int ada_check_table(const char* who, int64_t iteration, int64_t pass, int64_t rank, int64_t rows, int64_t H, int32_t policy) {
  if (int rc = aug_check_key(who, iteration, pass, rank, rows, 0x7fffffff / CSG_ADA_ROW_WORDS, "0 .. 2^26 - 1")) return rc;
  if (int rc = aug_check_h(who, H)) return rc;
  CSG_REQUIRE(policy >= 0 && policy < 64, CSG_E_BADSHAPE,
              "%s: policy %d (a sum of 8 = ada_blit, 16 = ada_geom, 32 = ada_color; the bits below count for nothing)", who,
              (int)policy);
  return CSG_OK;
}

template <bool BWD>
static int ada_apply(const char* who, const float* in, float* out, const uint32_t* table, int64_t table_rows, int64_t N, int64_t H,
                     int64_t Ct, int64_t c0, void* stream) {
  bool empty;
  if (int rc = aug_check_map(who, in, out, table, table_rows, N, H, Ct, c0, "a resampled pixel reads other ones", empty)) return rc;
  if (empty) return CSG_OK;
  hipStream_t s = (hipStream_t)stream;
  const unsigned total4 = (unsigned)(N * H * H * (Ct / 4));
  const unsigned grid = (unsigned)cdiv((int64_t)total4, (int64_t)kAdaThreads);
  ProfScope p(K_AUGMENT, (double)N * H * H * Ct * 8.0, s);
  if (BWD) CSG_LAUNCH(k_ada_pipeline_bwd, dim3(grid), dim3(kAdaThreads), 0, s, in, out, table, (int)H, (int)Ct, (int)c0, total4);
  else CSG_LAUNCH(k_ada_pipeline_fwd, dim3(grid), dim3(kAdaThreads), 0, s, in, out, table, (int)H, (int)Ct, (int)c0, total4);
  return check_launch(who);
}

}  // namespace csg

using namespace csg;

extern "C" {

int csg_ada_pipeline_table_host(uint64_t seed, int64_t iteration, int64_t pass, int64_t rank, int64_t rows, int64_t H,
                                int32_t policy, int64_t p24, uint32_t* table) {
  if (int rc = ada_check_table("csg_ada_pipeline_table_host", iteration, pass, rank, rows, H, policy)) return rc;
  if (int rc = aug_check_p24("csg_ada_pipeline_table_host", p24)) return rc;
  CSG_REQUIRE(rows == 0 || table != nullptr, CSG_E_BADSHAPE, "csg_ada_pipeline_table_host: null table");
  for (int64_t n = 0; n < rows; ++n) {
    const AdaRow r = ada_row(seed, (uint64_t)iteration, (uint64_t)pass, (uint64_t)rank, (uint64_t)n, (int32_t)H, policy, (uint32_t)p24);
    for (int k = 0; k < CSG_ADA_ROW_WORDS; ++k) table[CSG_ADA_ROW_WORDS * n + k] = r.w[k];
  }
  return CSG_OK;
}

int csg_ada_pipeline_table(uint64_t seed, int64_t iteration, int64_t pass, int64_t rank, int64_t rows, int64_t H, int32_t policy,
                           const int64_t* ctrl, uint32_t* table, void* stream) {
  if (int rc = ada_check_table("csg_ada_pipeline_table", iteration, pass, rank, rows, H, policy)) return rc;
  if (int rc = aug_check_ctrl("csg_ada_pipeline_table", ctrl)) return rc;
  if (rows == 0) return CSG_OK;
  CSG_REQUIRE(table != nullptr && ((uintptr_t)table & 15) == 0, CSG_E_BADSHAPE,
              "csg_ada_pipeline_table: the table must be 16-byte aligned (null pointer or misaligned)");
  hipStream_t s = (hipStream_t)stream;
  CSG_LAUNCH(k_ada_pipeline_table, dim3((unsigned)cdiv(rows, (int64_t)kAdaThreads)), dim3(kAdaThreads), 0, s, seed,
             (uint64_t)iteration, (uint64_t)pass, (uint64_t)rank, (int)rows, (int)H, (int)policy, ctrl, table);
  return check_launch("csg_ada_pipeline_table");
}

int csg_ada_pipeline_fwd(const float* in, float* out, const uint32_t* table, int64_t table_rows, int64_t N, int64_t H, int64_t Ct,
                         int64_t c0, void* stream) {
  return ada_apply<false>("csg_ada_pipeline_fwd", in, out, table, table_rows, N, H, Ct, c0, stream);
}

int csg_ada_pipeline_bwd(const float* in, float* out, const uint32_t* table, int64_t table_rows, int64_t N, int64_t H, int64_t Ct,
                         int64_t c0, void* stream) {
  return ada_apply<true>("csg_ada_pipeline_bwd", in, out, table, table_rows, N, H, Ct, c0, stream);
}

}  // extern "C"
