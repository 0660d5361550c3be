// Host side of the augmentation entries (augment.hip, ada_pipeline.hip), written once: the checks of a hash key, of the map a
// transform runs on, of the controller's pointer and of p24.  Every check returns through CSG_REQUIRE with the entry's name
// in front; nothing here launches a kernel.
#pragma once
#include "csg_common.h"
#include "csg_augment.h"

namespace csg {

// The key of a table or gate fill.  `row_range` is the text of [0, max_rows] for the message.
static inline int aug_check_key(const char* who, int64_t iteration, int64_t pass, int64_t rank, int64_t rows, int64_t max_rows,
                                const char* row_range) {
  CSG_REQUIRE(iteration >= 0 && pass >= 0 && pass <= 0x7fffffff && rank >= 0 && rank <= 0x7fffffff, CSG_E_BADSHAPE,
              "%s: iteration %ld, pass %ld and rank %ld must be non-negative (pass and rank below 2^31)", who, (long)iteration,
              (long)pass, (long)rank);
  CSG_REQUIRE(rows >= 0 && rows <= max_rows, CSG_E_BADSHAPE, "%s: %ld rows (%s)", who, (long)rows, row_range);
  return CSG_OK;
}

static inline int aug_check_h(const char* who, int64_t H) {
  CSG_REQUIRE(H >= 2 && H <= CSG_AUG_MAX_H, CSG_E_BADSHAPE, "%s: H = %ld (2 .. %d)", who, (long)H, CSG_AUG_MAX_H);
  return CSG_OK;
}

// What a transform and its adjoint ask of (in, out, table): N samples of H x H x Ct floats, colour channels [c0, c0 + 3), one
// table row per sample.  `empty` is N == 0: the caller returns CSG_OK, and no pointer has been looked at.  `why` is the
// reason the map cannot run in place.
static inline int aug_check_map(const char* who, const float* in, const float* out, const uint32_t* table, int64_t table_rows,
                                int64_t N, int64_t H, int64_t Ct, int64_t c0, const char* why, bool& empty) {
  empty = N == 0;
  if (int rc = aug_check_h(who, H)) return rc;
  CSG_REQUIRE(Ct >= 4 && Ct % 4 == 0, CSG_E_BADSHAPE, "%s: Ct = %ld must be a positive multiple of 4 (16-byte pixel rows)", who,
              (long)Ct);
  CSG_REQUIRE(c0 >= 0 && c0 + 3 <= Ct, CSG_E_BADSHAPE, "%s: colour channels [%ld, %ld) do not fit Ct = %ld (c0 + 3 > Ct)", who,
              (long)c0, (long)c0 + 3, (long)Ct);
  CSG_REQUIRE(N >= 0 && N <= 0x7fffffff && (double)N * (double)H * (double)H * (double)Ct < 2147483648.0, CSG_E_BADSHAPE,
              "%s: N = %ld samples of %ld x %ld x %ld floats (fewer than 2^31 floats in all)", who, (long)N, (long)H, (long)H,
              (long)Ct);
  CSG_REQUIRE(table_rows >= N, CSG_E_BADSHAPE, "%s: the table has %ld rows, fewer than N = %ld", who, (long)table_rows, (long)N);
  if (empty) return CSG_OK;
  CSG_REQUIRE(in != nullptr && out != nullptr && table != nullptr, CSG_E_BADSHAPE, "%s: null pointer", who);
  CSG_REQUIRE((((uintptr_t)in | (uintptr_t)out | (uintptr_t)table) & 15) == 0, CSG_E_BADSHAPE,
              "%s: in, out and the table must be 16-byte aligned", who);
  CSG_REQUIRE((const void*)in != (const void*)out, CSG_E_BADSHAPE, "%s: not in place (%s)", who, why);
  return CSG_OK;
}

static inline int aug_check_ctrl(const char* who, const int64_t* ctrl) {
  CSG_REQUIRE(ctrl != nullptr && ((uintptr_t)ctrl & 7) == 0, CSG_E_BADSHAPE,
              "%s: the controller must be 8-byte aligned (null pointer or misaligned)", who);
  return CSG_OK;
}

static inline int aug_check_p24(const char* who, int64_t p24) {
  CSG_REQUIRE(p24 >= 0 && p24 <= CSG_ADA_ONE, CSG_E_BADSHAPE, "%s: p24 = %ld (0 .. 2^24)", who, (long)p24);
  return CSG_OK;
}

}  // namespace csg
