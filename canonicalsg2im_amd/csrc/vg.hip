// Visual Genome object rows -> object ids and boxes: the per-object loop of the reference's __getitem__
// (sg2im/data/packed_vg.py:110-125) and the padding of vg_collate_fn (:186-205) for a padded batch, one lane per
// (sample, object) row.
//
// The reference reads a row (name, x, y, w, h) of integers in pixels and the decoded picture's size (WW, HH), computes in
// Python floats (fp64) and rounds once, when the list becomes a FloatTensor (:118-120):
//     objs = name;   box = (float(x) / WW, float(y) / HH, float(w) / WW, float(h) / HH)
// Four divisions and one rounding each.  For integers below 2^24 a plain fp32 division gives the same bits (the fp64 quotient
// carries 53 >= 2 * 24 + 2 bits, so rounding it to fp32 cannot round twice); the fp64 form is kept so that this file reads
// like the reference and holds for any int32 row.  Compiled with -ffp-contract=off, like clevr.hip.
// A row at or beyond its sample's count is the collate's padding: objs = 0, box = (-1, -1, -1, -1).
#include "csg_common.h"

namespace csg {

constexpr int kVgThreads = 256;

// rows (B,O,5) int32 = name, x, y, w, h; sizes (B,2) = HH, WW; objs (B,O); boxes (B,O) float4.  The host refused names
// outside 1 .. num_names - 1 and sizes below 1 from its own copies; a device row that disagrees with them (a stale buffer
// under a replayed graph) becomes a padding row too.
__global__ __launch_bounds__(kVgThreads) void k_vg_rows(const int32_t* __restrict__ rows, const int64_t* __restrict__ sizes,
                                                        const int64_t* __restrict__ counts, int num_names, int B, int O,
                                                        int64_t* __restrict__ objs, float4* __restrict__ boxes) {
  const int i = blockIdx.x * kVgThreads + threadIdx.x;
  if (i >= B * O) return;
  const int b = i / O, o = i - b * O;
  const int32_t* r = rows + (int64_t)i * 5;
  const int32_t name = r[0];
  const int64_t HH = sizes[2 * b], WW = sizes[2 * b + 1];
  int64_t obj = 0;
  float4 box = make_float4(-1.f, -1.f, -1.f, -1.f);
  if ((int64_t)o < counts[b] && name >= 1 && name < num_names && HH >= 1 && WW >= 1) {
    const double ww = (double)WW, hh = (double)HH;
    obj = name;
    box = make_float4((float)((double)r[1] / ww), (float)((double)r[2] / hh), (float)((double)r[3] / ww),
                      (float)((double)r[4] / hh));
  }
  objs[i] = obj;
  boxes[i] = box;
}

}  // namespace csg

using namespace csg;

extern "C" {

int csg_vg_rows(const int32_t* rows, const int64_t* sizes, const int64_t* counts, const int32_t* rows_host,
                const int64_t* sizes_host, const int64_t* counts_host, int64_t num_object_names, int64_t B, int64_t O,
                int64_t* objs, float* boxes, void* stream) {
  CSG_REQUIRE(B >= 1 && B <= CSG_VG_MAX_BATCH && O >= 1 && O <= CSG_VG_MAX_OBJECTS, CSG_E_BADSHAPE,
              "csg_vg_rows: bad shape B=%ld O=%ld (1 <= B <= %d, 1 <= O <= %d: the canonical graph takes %d rows with __image__)",
              (long)B, (long)O, CSG_VG_MAX_BATCH, CSG_VG_MAX_OBJECTS, CSG_VG_MAX_OBJECTS + 1);
  CSG_REQUIRE(num_object_names >= 2 && num_object_names <= INT32_MAX, CSG_E_BADSHAPE,
              "csg_vg_rows: %ld object names, 2 .. 2^31 - 1 (__image__ and at least one more)", (long)num_object_names);
  CSG_REQUIRE(rows != nullptr && sizes != nullptr && counts != nullptr && rows_host != nullptr && sizes_host != nullptr &&
                  counts_host != nullptr && objs != nullptr && boxes != nullptr,
              CSG_E_BADSHAPE, "csg_vg_rows: null operand");
  CSG_REQUIRE(((uintptr_t)boxes & 15) == 0 && (((uintptr_t)sizes | (uintptr_t)counts | (uintptr_t)objs) & 7) == 0 &&
                  ((uintptr_t)rows & 3) == 0,
              CSG_E_BADSHAPE, "csg_vg_rows: boxes must be 16-byte aligned, the int64 operands 8-byte aligned, rows 4-byte aligned");
  for (int64_t b = 0; b < B; ++b) {
    const int64_t n = counts_host[b];
    CSG_REQUIRE(n >= 0 && n <= O, CSG_E_BADSHAPE, "csg_vg_rows: sample %ld has %ld objects, 0 .. O = %ld", (long)b, (long)n,
                (long)O);
    CSG_REQUIRE(sizes_host[2 * b] >= 1 && sizes_host[2 * b + 1] >= 1, CSG_E_BADSHAPE,
                "csg_vg_rows: the picture of sample %ld is %ld x %ld (HH x WW), at least 1 x 1", (long)b, (long)sizes_host[2 * b],
                (long)sizes_host[2 * b + 1]);
    for (int64_t o = 0; o < n; ++o) {
      const int64_t name = rows_host[(b * O + o) * 5];
      CSG_REQUIRE(name >= 1 && name < num_object_names, CSG_E_BADSHAPE,
                  "csg_vg_rows: object %ld of sample %ld has name id %ld, 1 .. %ld", (long)o, (long)b, (long)name,
                  (long)(num_object_names - 1));
    }
  }
  hipStream_t s = (hipStream_t)stream;
  ProfScope p(K_VG_ROWS, (double)B * O * (5 * 4 + 8 + 16), s);
  CSG_LAUNCH(k_vg_rows, dim3((unsigned)cdiv(B * O, kVgThreads)), dim3(kVgThreads), 0, s, rows, sizes, counts,
             (int)num_object_names, (int)B, (int)O, objs, (float4*)boxes);
  return check_launch("csg_vg_rows");
}

}  // extern "C"
