// CLEVR scene geometry -> object boxes: the reference's extract_bounding_boxes (sg2im/data/packed_clevr_dialog.py:21-77)
// for a padded batch, one lane per object.
//
// The reference works in Python floats (fp64) and rounds once, when the lists become a FloatTensor.  Per object, with
// (x, y) = pixel_coords[:2], (x1, y1, z1) = 3d_coords and (cos, sin) = directions['right'][:2] of its scene:
//     x1 = x1 * cos + y1 * sin;   y1 = x1 * -sin + y1 * cos          (the second line reads the NEW x1: kept)
//     r  = 6.9 * z1 * (15 - y1) / 2.0                                  (left to right);  up = down = left = right = r
//     cylinder:  d = 9.4 + y1, h = 6.4, s = z1
//                up   *= (s * (h / d + 1)) / ((s * (h / d + 1)) - (s * (h - s) / d))
//                down  = up * (h - s + d) / (h + s + d)
//                left *= 11 / (10 + y1);  right = left
//     cube:      up *= 1.3 * 10 / (10 + y1)   ((1.3 * 10) first);  down = left = right = up
//     y_min = (y - down) / 320, y_max = (y + up) / 320, x_max = (x + right) / 480, x_min = (x - left) / 480
//     box = (x_min, y_min, x_max - x_min, y_max - y_min)
// The divisors are 320 and 480 whatever the picture's size.  Only + - * / occur; this file is compiled with
// -ffp-contract=off, so every operation is the correctly rounded one the host performs and the fp32 rows EQUAL the reference's.
#include "csg_common.h"

namespace csg {

constexpr int kClevrThreads = 256;
constexpr int kClevrCube = 1, kClevrSphere = 2, kClevrCylinder = 3;      // vocab["attributes"]["shape"] (:121)

__device__ __forceinline__ float4 clevr_box(double x, double y, double x1, double y1, double z1, double cos_t, double sin_t,
                                            int shape) {
  x1 = x1 * cos_t + y1 * sin_t;
  y1 = x1 * -sin_t + y1 * cos_t;
  double down = 6.9 * z1 * (15.0 - y1) / 2.0;
  double up = down, left = down, right = down;
  if (shape == kClevrCylinder) {
    const double d = 9.4 + y1;
    const double h = 6.4;
    const double s = z1;
    up = up * ((s * (h / d + 1.0)) / ((s * (h / d + 1.0)) - (s * (h - s) / d)));
    down = up * (h - s + d) / (h + s + d);
    left = left * (11.0 / (10.0 + y1));
    right = left;
  }
  if (shape == kClevrCube) {
    up = up * (1.3 * 10.0 / (10.0 + y1));
    down = up;
    left = up;
    right = up;
  }
  const double y_min = (y - down) / 320.0;
  const double y_max = (y + up) / 320.0;
  const double x_max = (x + right) / 480.0;
  const double x_min = (x - left) / 480.0;
  return make_float4((float)x_min, (float)y_min, (float)(x_max - x_min), (float)(y_max - y_min));
}

// boxes (B,O,4).  A row at or beyond its scene's count is padding: -1.  The host refused shape ids outside 1..3 from its
// own copy; a device row that disagrees with it (a stale buffer under a replayed graph) becomes a padding row too.
__global__ __launch_bounds__(kClevrThreads) void k_clevr_boxes(const double* __restrict__ geom, const int64_t* __restrict__ objs,
                                                               int A, const double* __restrict__ rot,
                                                               const int64_t* __restrict__ counts, int B, int O,
                                                               float4* __restrict__ boxes) {
  const int i = blockIdx.x * kClevrThreads + threadIdx.x;
  if (i >= B * O) return;
  const int b = i / O, o = i - b * O;
  const int64_t shape = objs[(int64_t)i * A];
  float4 box = make_float4(-1.f, -1.f, -1.f, -1.f);
  if ((int64_t)o < counts[b] && shape >= kClevrCube && shape <= kClevrCylinder) {
    const double* g = geom + (int64_t)i * 5;
    box = clevr_box(g[0], g[1], g[2], g[3], g[4], rot[2 * b], rot[2 * b + 1], (int)shape);
  }
  boxes[i] = box;
}

}  // namespace csg

using namespace csg;

extern "C" {

int csg_clevr_boxes(const double* geom, const int64_t* objs, int64_t A, const double* rot, const int64_t* counts,
                    const int64_t* objs_host, const int64_t* counts_host, int64_t B, int64_t O, float* boxes, void* stream) {
  CSG_REQUIRE(B >= 1 && B <= CSG_CLEVR_MAX_BATCH && O >= 1 && O <= CSG_CLEVR_MAX_OBJECTS && A >= 1 && A <= 64, CSG_E_BADSHAPE,
              "csg_clevr_boxes: bad shape B=%ld O=%ld A=%ld (B <= %d, O <= %d, A <= 64)", (long)B, (long)O, (long)A,
              CSG_CLEVR_MAX_BATCH, CSG_CLEVR_MAX_OBJECTS);
  CSG_REQUIRE(geom != nullptr && objs != nullptr && rot != nullptr && counts != nullptr && objs_host != nullptr &&
                  counts_host != nullptr && boxes != nullptr,
              CSG_E_BADSHAPE, "csg_clevr_boxes: null operand");
  CSG_REQUIRE(((uintptr_t)boxes & 15) == 0 && (((uintptr_t)geom | (uintptr_t)rot | (uintptr_t)objs | (uintptr_t)counts) & 7) == 0,
              CSG_E_BADSHAPE, "csg_clevr_boxes: boxes must be 16-byte aligned, the fp64 and int64 inputs 8-byte aligned");
  for (int64_t b = 0; b < B; ++b) {
    const int64_t n = counts_host[b];
    CSG_REQUIRE(n >= 0 && n <= O, CSG_E_BADSHAPE, "csg_clevr_boxes: scene %ld has %ld objects, 0 .. O = %ld", (long)b, (long)n,
                (long)O);
    for (int64_t o = 0; o < n; ++o) {
      const int64_t shape = objs_host[(b * O + o) * A];
      CSG_REQUIRE(shape >= kClevrCube && shape <= kClevrCylinder, CSG_E_BADSHAPE,
                  "csg_clevr_boxes: object %ld of scene %ld has shape id %ld, 1 (cube) .. 3 (cylinder)", (long)o, (long)b,
                  (long)shape);
    }
  }
  hipStream_t s = (hipStream_t)stream;
  ProfScope p(K_CLEVR_BOXES, (double)B * O * (5 * 8 + 8 + 16), s);
  CSG_LAUNCH(k_clevr_boxes, dim3((unsigned)cdiv(B * O, kClevrThreads)), dim3(kClevrThreads), 0, s, geom, objs, (int)A, rot, counts,
             (int)B, (int)O, (float4*)boxes);
  return check_launch("csg_clevr_boxes");
}

}  // extern "C"
