// The ADA augmentation pipeline (StyleGAN2-ADA, Karras et al., NeurIPS 2020, appendix B) of what the discriminators see
// (ada_pipeline.hip): the parameter row of one sample, written ONCE for the host and the device.  Integers and fp64 with
// separate multiplications and additions only (the file that includes this header is compiled with -ffp-contract=off), no
// libm: what the host computes and what a kernel computes are the same bits, and tests/ada_pipeline_cases.py restates them
// in numpy uint64 / float64.
//
// DRAWS.  key h = aug_key(seed, iteration, pass, rank, n) of csg_augment.h; draw k = step(h, k).  Draws 1..10 are
// DiffAugment's rows and gates and stay what they are; the pipeline's draws start at 16.  Every draw exists whether or not its
// group is on: switching one group does not move the others.
//     16 x-flip gate      17 x-flip i (top bit)         18 rot90 gate       19 rot90 k (top two bits)
//     20 shift gate       21 tx   22 ty                 23 iso gate         24..35 iso z
//     36 pre-rot gate     37 pre-rot angle              38 aniso gate       39..50 aniso z
//     51 post-rot gate    52 post-rot angle             53 frac gate        54..65 frac z_x    66..77 frac z_y
//     78 brightness gate  79..90 z                      91 contrast gate    92..103 z
//     104 luma gate       105 luma i (top bit)          106 hue gate        107 hue angle
//     108 saturation gate 109..120 z
// A gate is on iff aug_u24(draw) < p24; the two rotations' gates compare with
//     prot24 = floor((1 - sqrt(1 - p24 2^-24)) 2^24)          (fp64; the square root is correctly rounded on both sides)
// so that at least one of them is on with probability p.  An angle is the draw's 24 bits as a fraction of a turn.
// z, the "normal": the exact integer sum of twelve 24-bit draws minus 6 2^24, times 2^-24 (exact in fp64): mean 0, variance 1,
// |z| <= 6 — an Irwin-Hall sum, NOT a true normal (no tails beyond 6 sigma).
//
// PARAMETERS (appendix B).  x-flip i in {0, 1}; rot90 k in {0..3}; tx, ty = aug_int(draw, 2 t + 1) - t, t = (H + 4) >> 3;
// isotropic scale 2^e, e = clamp(0.2 z, -1, 1); anisotropic scale (2^e, 2^-e), e likewise — the clamp is a deviation: the
// magnification stays <= 4 per axis and the adjoint's search box has a compile-time bound; fractional shift (0.125 H) z per
// axis; brightness 0.2 z; contrast 2^(0.5 z); luma flip I - 2 v v^T i, v = (1, 1, 1) / sqrt(3); hue: the rotation about v by
// the angle; saturation v v^T + (I - v v^T) 2^z.
//
// MATHS.  exp2(e): n = (int)floor(e + 0.5), f = e - n in [-1/2, 1/2], t = f ln2, the Taylor polynomial of e^t through t^14 by
// Horner (separate * and +), times the exact power of two 2^n made from its exponent bits.  sin, cos of u 2^-24 turns: the top
// three bits pick the octant o = u >> 21 and the nearest quarter turn q = ((o + 1) >> 1) & 3; the remainder
// r = u - (((o + 1) >> 1) << 22) in [-2^21, 2^21) gives phi = r (2 pi 2^-24) in [-pi/4, pi/4); sin phi through phi^17 and
// cos phi through phi^18 by Horner in phi^2; the quarter turn permutes and negates the pair.  Remainders are below 1e-19.
//
// COMPOSITION, fp64, in coordinates about the centre c = (H - 1) / 2 (x' = x - c).  An affine map is (l00 l01 t0; l10 l11 t1);
//     (A o B).l_ij = A.l_i0 * B.l_0j + A.l_i1 * B.l_1j          (A o B).t_i = (A.l_i0 * B.t_0 + A.l_i1 * B.t_1) + A.t_i
// M, output pixel -> source coordinate, starts as the identity and takes M <- M o X^-1 for each transform X that is on, in the
// order x-flip, rot90, shift, iso, pre-rot, aniso, post-rot, frac; G, the forward map, takes G <- X o G.  A transform that is
// off is skipped.  x-flip: diag(-1, 1).  rot90 by k quarter turns is numpy's rot90(a, k) of the (y, x) axes: the inverse has
// l = (ck -sk; sk ck), (ck, sk) = (1,0), (0,1), (-1,0), (0,-1).  Shift: out[y, x] = in[y - ty, x - tx].  Rotation by an
// angle: forward l = (c -s; s c).  Scales: forward diag(2^e, 2^e) and diag(2^e, 2^-e); the inverses use 2^-e from the same
// polynomial, no division.  The colour matrix C (3 x 4, on (r, g, b, 1)) starts as the identity and takes C <- A o C with
//     (A o C).l_ij = (A.l_i0 * C.l_0j + A.l_i1 * C.l_1j) + A.l_i2 * C.l_2j
//     (A o C).t_i  = ((A.l_i0 * C.t_0 + A.l_i1 * C.t_1) + A.l_i2 * C.t_2) + A.t_i
// in the order brightness (t = b), contrast (l = diag c), luma flip (off = -2 third, diag = 1 + off, third = 1.0 / 3.0), hue
// (a = (1 - cos) third, b = sin / sqrt(3): diag cos + a, off a -+ b) and saturation (off = third - third s, diag = off + s).
// Every stored entry is rounded ONCE to fp32: m02 = (float)(M.t0 + c), and likewise m12, g02, g12.
//
// THE ROW: CSG_ADA_ROW_WORDS = 32 words of 32 bits, 16-byte aligned:
//     0..5    M = m00 m01 m02 m10 m11 m12, fp32:  sx = (m00 x' + m01 y') + m02,  sy = (m10 x' + m11 y') + m12
//     6..11   G = g00 .. g12, fp32, the forward map in the same form (source pixel -> output coordinate)
//     12      the adjoint's search margin, int32 (1 for generated rows; the kernel clamps it to [0, CSG_ADA_MAX_MARGIN])
//     13      flags: CSG_ADA_GEOM_ID | CSG_ADA_GEOM_INT | CSG_ADA_COLOR_ID
//     14, 15  ex, ey, int32: the integer map's offsets
//     16..27  C = c00 c01 c02 c03 | c10 .. | c20 .., fp32:  r' = ((c00 r + c01 g) + c02 b) + c03
//     28..31  a b c d, int32, a signed permutation: the integer map  sx = a x + b y + ex,  sy = c x + d y + ey
// CSG_ADA_GEOM_INT is set when no general geometric transform is on for the sample (the geometry is then x-flip, rot90 and the
// integer shift: a signed permutation and a shift, applied as a copy); CSG_ADA_GEOM_ID when none of those three is on either;
// CSG_ADA_COLOR_ID when no colour transform is on.  A sample with all three is a bit copy.
//
// THE SEARCH BOX of the adjoint (ada_pipeline.hip): for a source pixel q the output pixels whose taps can hold q lie in the
// bounding box of G (q + (-1, 1)^2): centre G q, half sides |g00| + |g01| and |g10| + |g11|, widened by the margin.  The
// linear part of a generated G has singular values <= 4, so a half side is <= 4 sqrt(2) < 5.66 and a side of the box is at most
// floor(2 * 5.66 + 2) + 1 + 2 * 1 = 16 = CSG_ADA_MAX_BOX pixels.
#pragma once
#include <stdint.h>
#include <string.h>

#include "csg_augment.h"

#define CSG_ADA_ROW_WORDS 32
#define CSG_ADA_MAX_BOX 16
#define CSG_ADA_MAX_MARGIN 4
#define CSG_ADA_GEOM_ID 1
#define CSG_ADA_GEOM_INT 2
#define CSG_ADA_COLOR_ID 4
#define CSG_ADA_FIRST_DRAW 16

namespace csg {

struct AdaRow {
  uint32_t w[CSG_ADA_ROW_WORDS];
};

struct AdaAff {
  double l00, l01, t0, l10, l11, t1;
};

struct AdaCol {
  double l[3][3], t[3];
};

CSG_AUG_HD double ada_bits_f64(uint64_t u) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __longlong_as_double((long long)u);
#else
  double d;
  memcpy(&d, &u, 8);
  return d;
#endif
}

CSG_AUG_HD double ada_sqrt(double a) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __dsqrt_rn(a);
#else
  return __builtin_sqrt(a);
#endif
}

CSG_AUG_HD double ada_floor(double a) {
#if defined(__HIP_DEVICE_COMPILE__)
  return floor(a);
#else
  return __builtin_floor(a);
#endif
}

// p24 in [0, 2^24]
CSG_AUG_HD uint32_t ada_prot24(uint32_t p24) {
  const double a = 1.0 - (double)p24 * 5.9604644775390625e-08;          // exact
  const double r = 1.0 - ada_sqrt(a);
  return (uint32_t)ada_floor(r * 16777216.0);
}

// |e| <= 64
CSG_AUG_HD double ada_exp2(double e) {
  const double nf = ada_floor(e + 0.5);
  const double f = e - nf;                                              // exact: [-1/2, 1/2]
  const double t = f * 0.6931471805599453094;
  double p = 1.0 / 87178291200.0;                                       // 1 / 14!
  p = p * t + 1.0 / 6227020800.0;
  p = p * t + 1.0 / 479001600.0;
  p = p * t + 1.0 / 39916800.0;
  p = p * t + 1.0 / 3628800.0;
  p = p * t + 1.0 / 362880.0;
  p = p * t + 1.0 / 40320.0;
  p = p * t + 1.0 / 5040.0;
  p = p * t + 1.0 / 720.0;
  p = p * t + 1.0 / 120.0;
  p = p * t + 1.0 / 24.0;
  p = p * t + 1.0 / 6.0;
  p = p * t + 0.5;
  p = p * t + 1.0;
  p = p * t + 1.0;
  return p * ada_bits_f64((uint64_t)(1023 + (int64_t)nf) << 52);
}

// u: 24 bits, a fraction of a turn
CSG_AUG_HD void ada_sincos(uint32_t u, double& s, double& c) {
  const uint32_t h = ((u >> 21) + 1u) >> 1;                             // the nearest quarter turn, 0..4
  const int32_t r = (int32_t)u - (int32_t)(h << 22);
  const double phi = (double)r * (6.283185307179586476925 * 5.9604644775390625e-08);    // 2 pi 2^-24
  const double x = phi * phi;
  double ps = -1.0 / 355687428096000.0;                                 // -1 / 17!
  ps = ps * x + 1.0 / 1307674368000.0;
  ps = ps * x + -1.0 / 6227020800.0;
  ps = ps * x + 1.0 / 39916800.0;
  ps = ps * x + -1.0 / 362880.0;
  ps = ps * x + 1.0 / 5040.0;
  ps = ps * x + -1.0 / 120.0;
  ps = ps * x + 1.0 / 6.0;
  ps = ps * x;
  const double sp = phi - phi * ps;                                     // phi (1 - x / 6 + ...)
  double pc = -1.0 / 6402373705728000.0;                                // -1 / 18!
  pc = pc * x + 1.0 / 20922789888000.0;
  pc = pc * x + -1.0 / 87178291200.0;
  pc = pc * x + 1.0 / 479001600.0;
  pc = pc * x + -1.0 / 3628800.0;
  pc = pc * x + 1.0 / 40320.0;
  pc = pc * x + -1.0 / 720.0;
  pc = pc * x + 1.0 / 24.0;
  pc = pc * x + -0.5;
  const double cp = pc * x + 1.0;
  switch (h & 3u) {
    case 0: s = sp; c = cp; break;
    case 1: s = cp; c = -sp; break;
    case 2: s = -sp; c = -cp; break;
    default: s = -cp; c = sp; break;
  }
}

CSG_AUG_HD AdaAff ada_aff_mul(const AdaAff& A, const AdaAff& B) {
  AdaAff R;
  R.l00 = A.l00 * B.l00 + A.l01 * B.l10;
  R.l01 = A.l00 * B.l01 + A.l01 * B.l11;
  R.t0 = (A.l00 * B.t0 + A.l01 * B.t1) + A.t0;
  R.l10 = A.l10 * B.l00 + A.l11 * B.l10;
  R.l11 = A.l10 * B.l01 + A.l11 * B.l11;
  R.t1 = (A.l10 * B.t0 + A.l11 * B.t1) + A.t1;
  return R;
}

CSG_AUG_HD AdaCol ada_col_mul(const AdaCol& A, const AdaCol& C) {
  AdaCol R;
  for (int i = 0; i < 3; ++i) {
    for (int j = 0; j < 3; ++j) R.l[i][j] = (A.l[i][0] * C.l[0][j] + A.l[i][1] * C.l[1][j]) + A.l[i][2] * C.l[2][j];
    R.t[i] = ((A.l[i][0] * C.t[0] + A.l[i][1] * C.t[1]) + A.l[i][2] * C.t[2]) + A.t[i];
  }
  return R;
}

CSG_AUG_HD AdaAff ada_aff(double l00, double l01, double t0, double l10, double l11, double t1) {
  AdaAff A;
  A.l00 = l00; A.l01 = l01; A.t0 = t0; A.l10 = l10; A.l11 = l11; A.t1 = t1;
  return A;
}

CSG_AUG_HD AdaCol ada_col(double diag, double off, double t) {
  AdaCol A;
  for (int i = 0; i < 3; ++i) {
    for (int j = 0; j < 3; ++j) A.l[i][j] = i == j ? diag : off;
    A.t[i] = t;
  }
  return A;
}

// the sum of the twelve draws first .. first + 11, as z
CSG_AUG_HD double ada_normal(uint64_t h, uint64_t first) {
  int64_t sum = 0;
  for (uint64_t k = 0; k < 12; ++k) sum += (int64_t)aug_u24(rw_step(h, first + k));
  return (double)(sum - 6 * CSG_ADA_ONE) * 5.9604644775390625e-08;
}

CSG_AUG_HD double ada_clamp1(double e) { return e < -1.0 ? -1.0 : e > 1.0 ? 1.0 : e; }

// H in [2, CSG_AUG_MAX_H], p24 in [0, 2^24], policy: a sum of CSG_AUG_ADA_BLIT / _GEOM / _COLOR (other bits count for nothing)
CSG_AUG_HD AdaRow ada_row(uint64_t seed, uint64_t iteration, uint64_t pass, uint64_t rank, uint64_t n, int32_t H, int32_t policy,
                          uint32_t p24) {
  const uint64_t h = aug_key(seed, iteration, pass, rank, n);
  const uint32_t prot24 = ada_prot24(p24);
  const bool blit = (policy & CSG_AUG_ADA_BLIT) != 0, geom = (policy & CSG_AUG_ADA_GEOM) != 0,
             colour = (policy & CSG_AUG_ADA_COLOR) != 0;
#define CSG_ADA_ON(k, thr) (aug_u24(rw_step(h, (uint64_t)(k))) < (thr))
  AdaAff M = ada_aff(1.0, 0.0, 0.0, 0.0, 1.0, 0.0), G = M;
  bool any_blit = false, any_geom = false, any_colour = false;
  // ---- pixel blitting
  if (blit && CSG_ADA_ON(16, p24)) {
    any_blit = true;
    if (rw_step(h, 17ull) >> 63) {
      const AdaAff F = ada_aff(-1.0, 0.0, 0.0, 0.0, 1.0, 0.0);
      M = ada_aff_mul(M, F);
      G = ada_aff_mul(F, G);
    }
  }
  if (blit && CSG_ADA_ON(18, p24)) {
    any_blit = true;
    const int k = (int)(rw_step(h, 19ull) >> 62);
    if (k) {
      const double ck = k == 2 ? -1.0 : 0.0, sk = k == 1 ? 1.0 : k == 3 ? -1.0 : 0.0;
      M = ada_aff_mul(M, ada_aff(ck, -sk, 0.0, sk, ck, 0.0));
      G = ada_aff_mul(ada_aff(ck, sk, 0.0, -sk, ck, 0.0), G);
    }
  }
  if (blit && CSG_ADA_ON(20, p24)) {
    any_blit = true;
    const int32_t t = (H + 4) >> 3;
    const double tx = (double)(aug_int(rw_step(h, 21ull), (uint32_t)(2 * t + 1)) - t);
    const double ty = (double)(aug_int(rw_step(h, 22ull), (uint32_t)(2 * t + 1)) - t);
    M = ada_aff_mul(M, ada_aff(1.0, 0.0, -tx, 0.0, 1.0, -ty));
    G = ada_aff_mul(ada_aff(1.0, 0.0, tx, 0.0, 1.0, ty), G);
  }
  // the integer map of the blit stage alone: entries of M are exact small integers here, c is a multiple of 1/2
  const double c = (double)(H - 1) * 0.5;
  const int32_t ia = (int32_t)M.l00, ib = (int32_t)M.l01, ic = (int32_t)M.l10, id = (int32_t)M.l11;
  const int32_t ex = (int32_t)((c - (M.l00 * c + M.l01 * c)) + M.t0), ey = (int32_t)((c - (M.l10 * c + M.l11 * c)) + M.t1);
  // ---- general geometry
  if (geom && CSG_ADA_ON(23, p24)) {
    any_geom = true;
    const double e = ada_clamp1(0.2 * ada_normal(h, 24ull));
    const double s = ada_exp2(e), si = ada_exp2(-e);
    M = ada_aff_mul(M, ada_aff(si, 0.0, 0.0, 0.0, si, 0.0));
    G = ada_aff_mul(ada_aff(s, 0.0, 0.0, 0.0, s, 0.0), G);
  }
  if (geom && CSG_ADA_ON(36, prot24)) {
    any_geom = true;
    double sn, cs;
    ada_sincos(aug_u24(rw_step(h, 37ull)), sn, cs);
    M = ada_aff_mul(M, ada_aff(cs, sn, 0.0, -sn, cs, 0.0));
    G = ada_aff_mul(ada_aff(cs, -sn, 0.0, sn, cs, 0.0), G);
  }
  if (geom && CSG_ADA_ON(38, p24)) {
    any_geom = true;
    const double e = ada_clamp1(0.2 * ada_normal(h, 39ull));
    const double s = ada_exp2(e), si = ada_exp2(-e);
    M = ada_aff_mul(M, ada_aff(si, 0.0, 0.0, 0.0, s, 0.0));
    G = ada_aff_mul(ada_aff(s, 0.0, 0.0, 0.0, si, 0.0), G);
  }
  if (geom && CSG_ADA_ON(51, prot24)) {
    any_geom = true;
    double sn, cs;
    ada_sincos(aug_u24(rw_step(h, 52ull)), sn, cs);
    M = ada_aff_mul(M, ada_aff(cs, sn, 0.0, -sn, cs, 0.0));
    G = ada_aff_mul(ada_aff(cs, -sn, 0.0, sn, cs, 0.0), G);
  }
  if (geom && CSG_ADA_ON(53, p24)) {
    any_geom = true;
    const double a = 0.125 * (double)H;
    const double tx = a * ada_normal(h, 54ull), ty = a * ada_normal(h, 66ull);
    M = ada_aff_mul(M, ada_aff(1.0, 0.0, -tx, 0.0, 1.0, -ty));
    G = ada_aff_mul(ada_aff(1.0, 0.0, tx, 0.0, 1.0, ty), G);
  }
  // ---- colour
  const double third = 1.0 / 3.0;
  AdaCol C = ada_col(1.0, 0.0, 0.0);
  if (colour && CSG_ADA_ON(78, p24)) {
    any_colour = true;
    C = ada_col_mul(ada_col(1.0, 0.0, 0.2 * ada_normal(h, 79ull)), C);
  }
  if (colour && CSG_ADA_ON(91, p24)) {
    any_colour = true;
    C = ada_col_mul(ada_col(ada_exp2(0.5 * ada_normal(h, 92ull)), 0.0, 0.0), C);
  }
  if (colour && CSG_ADA_ON(104, p24)) {
    any_colour = true;
    if (rw_step(h, 105ull) >> 63) {
      const double off = -2.0 * third;                                  // I - 2 v v^T
      C = ada_col_mul(ada_col(1.0 + off, off, 0.0), C);
    }
  }
  if (colour && CSG_ADA_ON(106, p24)) {
    any_colour = true;
    double sn, cs;
    ada_sincos(aug_u24(rw_step(h, 107ull)), sn, cs);
    const double a = (1.0 - cs) * third, b = sn * 0.57735026918962576451;   // 1 / sqrt(3)
    AdaCol R = ada_col(cs + a, 0.0, 0.0);
    R.l[0][1] = a - b; R.l[0][2] = a + b;
    R.l[1][0] = a + b; R.l[1][2] = a - b;
    R.l[2][0] = a - b; R.l[2][1] = a + b;
    C = ada_col_mul(R, C);
  }
  if (colour && CSG_ADA_ON(108, p24)) {
    any_colour = true;
    const double s = ada_exp2(ada_normal(h, 109ull));
    const double off = third - third * s;                               // v v^T + (I - v v^T) s
    C = ada_col_mul(ada_col(off + s, off, 0.0), C);
  }
#undef CSG_ADA_ON
  AdaRow r;
  r.w[0] = aug_float_bits((float)M.l00); r.w[1] = aug_float_bits((float)M.l01); r.w[2] = aug_float_bits((float)(M.t0 + c));
  r.w[3] = aug_float_bits((float)M.l10); r.w[4] = aug_float_bits((float)M.l11); r.w[5] = aug_float_bits((float)(M.t1 + c));
  r.w[6] = aug_float_bits((float)G.l00); r.w[7] = aug_float_bits((float)G.l01); r.w[8] = aug_float_bits((float)(G.t0 + c));
  r.w[9] = aug_float_bits((float)G.l10); r.w[10] = aug_float_bits((float)G.l11); r.w[11] = aug_float_bits((float)(G.t1 + c));
  r.w[12] = 1u;
  r.w[13] = (uint32_t)((any_geom ? 0 : CSG_ADA_GEOM_INT) | (any_geom || any_blit ? 0 : CSG_ADA_GEOM_ID) |
                       (any_colour ? 0 : CSG_ADA_COLOR_ID));
  r.w[14] = (uint32_t)ex;
  r.w[15] = (uint32_t)ey;
  for (int i = 0; i < 3; ++i) {
    for (int j = 0; j < 3; ++j) r.w[16 + 4 * i + j] = aug_float_bits((float)C.l[i][j]);
    r.w[16 + 4 * i + 3] = aug_float_bits((float)C.t[i]);
  }
  r.w[28] = (uint32_t)ia; r.w[29] = (uint32_t)ib; r.w[30] = (uint32_t)ic; r.w[31] = (uint32_t)id;
  return r;
}

}  // namespace csg
