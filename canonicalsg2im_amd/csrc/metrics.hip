// Box IoU of a padded validation batch: the reference's jaccard (sg2im/metrics.py:4-36) behind
// remove_dummies_and_padding (sg2im/utils.py:66-71) and the clamp of scripts/train.py:196, per object, with the sums
// check_model keeps (scripts/train.py:211-217).
//
// An object is COUNTED when any of its four ground-truth box values differs from -1 and objs[b,o,0] != __image__.  (This
// is not remove_dummy_objects, which tests objs[b,o,0] != 0: the reference uses two masks and so does this package.)
// Per counted object, every step one correctly rounded fp32 operation in the reference's order:
//     p = clamp(pred, 0, 1) as xywh;  corners (x, y, x + w, y + h) of p and of gt
//     inter = clamp(min(p1, g1) - max(p0, g0), min 0), its two extents multiplied
//     area = (x1 - x0) * (y1 - y0) of either box;  union = (area_pred + area_gt) - inter;  iou = inter / union
// This file is compiled with -ffp-contract=off (no multiply-add is formed from the products and the sum) and hipcc's
// default correctly rounded division: the bits are those of torch on the host.  min / max / clamp propagate NaN as torch's
// do; 0 / 0 (both boxes of zero area) is NaN, fails both comparisons and makes the sums NaN, as in the reference.
// The sums are fp64 in a fixed association (csg_reduce.h: strided lanes, wave tree, waves in order): no atomics, the
// same bits on every run.
#include "csg_common.h"
#include "csg_reduce.h"

namespace csg {

constexpr int kIouThreads = 256;

__device__ __forceinline__ float tmin(float a, float b) { return (a < b || a != a) ? a : b; }   // torch.min: NaN wins
__device__ __forceinline__ float tmax(float a, float b) { return (a > b || a != a) ? a : b; }
__device__ __forceinline__ float clamp01(float x) { return tmin(tmax(x, 0.f), 1.f); }

__device__ __forceinline__ float jaccard_one(float4 p, float4 g) {
  const float px0 = clamp01(p.x), py0 = clamp01(p.y), pw = clamp01(p.z), ph = clamp01(p.w);
  const float px1 = px0 + pw, py1 = py0 + ph;
  const float gx0 = g.x, gy0 = g.y;
  const float gx1 = gx0 + g.z, gy1 = gy0 + g.w;
  const float ix = tmax(tmin(px1, gx1) - tmax(px0, gx0), 0.f);
  const float iy = tmax(tmin(py1, gy1) - tmax(py0, gy0), 0.f);
  const float inter = ix * iy;
  const float area_p = (px1 - px0) * (py1 - py0);
  const float area_g = (gx1 - gx0) * (gy1 - gy0);
  const float uni = (area_p + area_g) - inter;
  return inter / uni;
}

// one block per sample, lanes strided over the O objects.  per_sample[b] = {sum iou, #iou > 0.5, #iou > 0.3, #counted}
__global__ __launch_bounds__(kIouThreads) void k_box_iou(const float4* __restrict__ pred, const float4* __restrict__ gt,
                                                         const int64_t* __restrict__ objs, int O, int A, int64_t image_id,
                                                         float* __restrict__ iou, uint8_t* __restrict__ counted,
                                                         double* __restrict__ per_sample) {
  __shared__ double part[kIouThreads / 64][4];
  const int b = blockIdx.x;
  const int64_t row = (int64_t)b * O;
  double acc[4] = {0.0, 0.0, 0.0, 0.0};
  for (int o = threadIdx.x; o < O; o += kIouThreads) {
    const float4 g = gt[row + o];
    const bool box = g.x != -1.f || g.y != -1.f || g.z != -1.f || g.w != -1.f;
    const bool on = box && objs[(row + o) * A] != image_id;
    float v = 0.f;
    if (on) {
      v = jaccard_one(pred[row + o], g);
      acc[0] += (double)v;
      acc[1] += v > 0.5f ? 1.0 : 0.0;
      acc[2] += v > 0.3f ? 1.0 : 0.0;
      acc[3] += 1.0;
    }
    iou[row + o] = v;
    counted[row + o] = on ? 1 : 0;
  }
  block_sum_f64<4, kIouThreads / 64>(acc, part);
  if (threadIdx.x == 0) {
#pragma unroll
    for (int q = 0; q < 4; ++q) per_sample[(int64_t)b * 4 + q] = acc[q];
  }
}

// totals[q] += sum_b per_sample[b][q]: one wave, lanes strided over the samples, the same tree
__global__ __launch_bounds__(64) void k_box_iou_fold(const double* __restrict__ per_sample, int B, double* __restrict__ totals) {
  __shared__ double part[1][4];
  double acc[4] = {0.0, 0.0, 0.0, 0.0};
  for (int b = threadIdx.x; b < B; b += 64) {
#pragma unroll
    for (int q = 0; q < 4; ++q) acc[q] += per_sample[(int64_t)b * 4 + q];
  }
  block_sum_f64<4, 1>(acc, part);
  if (threadIdx.x == 0) {
#pragma unroll
    for (int q = 0; q < 4; ++q) totals[q] = totals[q] + acc[q];
  }
}

}  // namespace csg

using namespace csg;

extern "C" {

int csg_box_iou(const float* boxes_pred, const float* boxes_gt, const int64_t* objs, int64_t B, int64_t O, int64_t A,
                int64_t image_id, float* iou, uint8_t* counted, double* per_sample, double* totals, void* stream) {
  CSG_REQUIRE(B > 0 && B <= 65535 && O > 0 && O <= (1 << 20) && A > 0 && A <= 64, CSG_E_BADSHAPE,
              "csg_box_iou: bad shape B=%ld O=%ld A=%ld (B <= 65535, O <= 2^20, A <= 64)", (long)B, (long)O, (long)A);
  CSG_REQUIRE(boxes_pred != nullptr && boxes_gt != nullptr && objs != nullptr && iou != nullptr && counted != nullptr &&
                  per_sample != nullptr && totals != nullptr,
              CSG_E_BADSHAPE, "csg_box_iou: null operand");
  CSG_REQUIRE(((uintptr_t)boxes_pred | (uintptr_t)boxes_gt) % 16 == 0 && ((uintptr_t)per_sample | (uintptr_t)totals) % 8 == 0,
              CSG_E_BADSHAPE, "csg_box_iou: boxes must be 16-byte aligned, the fp64 outputs 8-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  ProfScope p(K_BOX_IOU, (double)B * O * (32 + 8 + 5), s);
  CSG_LAUNCH(k_box_iou, dim3((unsigned)B), dim3(kIouThreads), 0, s, (const float4*)boxes_pred, (const float4*)boxes_gt, objs,
             (int)O, (int)A, image_id, iou, counted, per_sample);
  CSG_LAUNCH(k_box_iou_fold, dim3(1), dim3(64), 0, s, (const double*)per_sample, (int)B, totals);
  return check_launch("csg_box_iou");
}

}  // extern "C"
