// DiffAugment of the discriminators' inputs (augment.hip): the counter-based hash and the parameter row of one sample,
// written ONCE for the host and the device.  The hash is integers only (the splitmix64 step of csg_rewrite.h); the three
// floats of a row are made from integers by ONE int -> float conversion (round to nearest even, the same on both sides)
// and a multiplication by a power of two (exact), so what the host computes and what a kernel computes are the same bits,
// and tests/augment_cases.py restates them in numpy uint64 / float32.
//
//   key      h = step(step(step(step(0, seed), iteration), pass), row),   row = rank << 32 | n   (n: the sample's index in the
//            launch)
//   draw k   g_k = step(h, k), k = 1..7, in the order r1, r2, r3, tx, ty, cy, cx.  Every draw exists whether or not its policy
//            is on: switching one policy does not move the others.
//   float    u = g >> 40 (24 bits), r = u * 2^-24 in [0, 1)
//   integer  in [0, n):  ((g >> 32) * n) >> 32
//
//   b = r1 - 0.5   = float(u1 - 2^23) * 2^-24      exact (|u1 - 2^23| <= 2^23)
//   s = 2 * r2     = float(u2) * 2^-23             exact (u2 < 2^24)
//   c = r3 + 0.5   = float(u3 + 2^23) * 2^-24      u3 + 2^23 < 3 * 2^23 has up to 25 bits: the conversion rounds it once
//   t = int(H * 0.125 + 0.5) = (H + 4) >> 3;   tx = int(g4, 2t + 1) - t,  ty likewise from g5
//   size = int(H * 0.5 + 0.5) = (H + 1) >> 1;  centres cy, cx = int(g, H + (1 - size % 2)) in [0, H - 1 + (1 - size % 2)];
//   y0 = cy - size / 2, x0 = cx - size / 2
//
// A row is eight 32-bit words: the bits of b, s, c, then tx, ty, y0, x0, size as int32.
//
// THE GATE (adaptive strength, StyleGAN2-ADA's p): policy j = 0, 1, 2 (colour, translation, cutout) is on for the sample iff
//   aug_u24(step(h, 8 + j)) < p24,   p24 an integer in [0, 2^24] (p = p24 * 2^-24).
// Draws 8, 9, 10 are the gate's alone: draws 1..7 and every row are what they were.  p24 = 2^24 turns every policy on (a 24-bit
// draw is below 2^24), p24 = 0 turns every policy off.
//
// THE CONTROLLER is eight int64 words, [p24, S, C, updates, S_last, C_last, 0, 0]: S the sum of sign(D(real)) over the
// elements counted since the last update, C their number.  One update moves p24 by a fixed step towards the target:
//   d = S * 2^24 - T24 * C  (int64; the sign of S / C - T),   p24' = clamp(p24 + sgn(d) * step24, 0, 2^24);
// C = 0 or d = 0 leaves p24 alone.  |S| <= C < 2^38 keeps both products below 2^62; words outside that leave p24 alone too.
#pragma once
#include <stdint.h>
#include <string.h>

#include "csg_rewrite.h"

#if defined(__HIPCC__)
#define CSG_AUG_HD __host__ __device__ __forceinline__
#else
#define CSG_AUG_HD static inline
#endif

namespace csg {

struct AugRow {
  uint32_t w[8];
};

CSG_AUG_HD uint64_t aug_key(uint64_t seed, uint64_t iteration, uint64_t pass, uint64_t rank, uint64_t n) {
  uint64_t h = rw_step(0ull, seed);
  h = rw_step(h, iteration);
  h = rw_step(h, pass);
  return rw_step(h, (rank << 32) | n);
}

CSG_AUG_HD uint32_t aug_u24(uint64_t g) { return (uint32_t)(g >> 40); }
CSG_AUG_HD int32_t aug_int(uint64_t g, uint32_t n) { return (int32_t)(((g >> 32) * (uint64_t)n) >> 32); }

CSG_AUG_HD uint32_t aug_float_bits(float f) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __float_as_uint(f);
#else
  uint32_t u;
  memcpy(&u, &f, 4);
  return u;
#endif
}

// H in [2, 2^24]: the caller has refused everything else
CSG_AUG_HD AugRow aug_row(uint64_t seed, uint64_t iteration, uint64_t pass, uint64_t rank, uint64_t n, int32_t H) {
  const uint64_t h = aug_key(seed, iteration, pass, rank, n);
  const int32_t u1 = (int32_t)aug_u24(rw_step(h, 1ull));
  const int32_t u2 = (int32_t)aug_u24(rw_step(h, 2ull));
  const int32_t u3 = (int32_t)aug_u24(rw_step(h, 3ull));
  const int32_t t = (H + 4) >> 3;
  const int32_t size = (H + 1) >> 1;
  const uint32_t centres = (uint32_t)(H + (1 - size % 2));
  AugRow r;
  r.w[0] = aug_float_bits((float)(u1 - (1 << 23)) * 5.9604644775390625e-08f);   // 2^-24
  r.w[1] = aug_float_bits((float)u2 * 1.1920928955078125e-07f);                 // 2^-23
  r.w[2] = aug_float_bits((float)(u3 + (1 << 23)) * 5.9604644775390625e-08f);
  r.w[3] = (uint32_t)(aug_int(rw_step(h, 4ull), (uint32_t)(2 * t + 1)) - t);
  r.w[4] = (uint32_t)(aug_int(rw_step(h, 5ull), (uint32_t)(2 * t + 1)) - t);
  r.w[5] = (uint32_t)(aug_int(rw_step(h, 6ull), centres) - size / 2);
  r.w[6] = (uint32_t)(aug_int(rw_step(h, 7ull), centres) - size / 2);
  r.w[7] = (uint32_t)size;
  return r;
}

#define CSG_ADA_ONE (1ll << 24)
#define CSG_ADA_MAX_COUNT (1ll << 38)

// p24 in [0, 2^24]: the caller has clamped or refused everything else
CSG_AUG_HD uint32_t aug_gate(uint64_t seed, uint64_t iteration, uint64_t pass, uint64_t rank, uint64_t n, uint32_t p24) {
  const uint64_t h = aug_key(seed, iteration, pass, rank, n);
  uint32_t m = 0;
  for (uint32_t j = 0; j < 3; ++j)
    if (aug_u24(rw_step(h, 8ull + j)) < p24) m |= 1u << j;
  return m;
}

CSG_AUG_HD int64_t ada_clamp_p(int64_t p24) { return p24 < 0 ? 0 : p24 > CSG_ADA_ONE ? CSG_ADA_ONE : p24; }

CSG_AUG_HD int64_t ada_next_p(int64_t p24, int64_t S, int64_t C, int64_t T24, int64_t step24) {
  if (C <= 0 || C >= CSG_ADA_MAX_COUNT || S > C || S < -C) return p24;
  const int64_t d = S * CSG_ADA_ONE - T24 * C;
  if (d == 0) return p24;
  // step24 may be anything >= 1: saturate before the addition
  if (d > 0) return step24 >= CSG_ADA_ONE - p24 ? CSG_ADA_ONE : p24 + step24;
  return step24 >= p24 ? 0 : p24 - step24;
}

// one update of the record: p24 moves, (S, C) go to the _last words and start again from 0
CSG_AUG_HD void ada_update_words(int64_t* ctrl, int64_t T24, int64_t step24) {
  const int64_t S = ctrl[1], C = ctrl[2];
  ctrl[0] = ada_next_p(ada_clamp_p(ctrl[0]), S, C, T24, step24);
  ctrl[4] = S;
  ctrl[5] = C;
  ctrl[1] = 0;
  ctrl[2] = 0;
  ctrl[3] += 1;
}

}  // namespace csg
