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

}  // namespace csg
