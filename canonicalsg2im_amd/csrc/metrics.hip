// The device metrics of a padded batch: box IoU (below) and relation agreement (further down).
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

// ---- relation agreement: do predicted boxes obey the triplets they were laid out from? -------------------------------
// The datasets' location rule (base_dataset.py:42-81, canon.hip's pair loop) asked of one pair per triplet.  A row is
// TESTED when its predicate is one of the six location ids, its type is 0..3 and s, o are rows of the batch; it AGREES
// when the rule, on the clamped boxes and the centres, yields that predicate.  The counts are integers: two 32-bit halves
// of one 64-bit accumulator per (type, relation), {agreeing << 32 | tested}, summed by fixed trees (lanes strided over
// the rows, a shuffle tree per wave, the waves in order); no atomics.
constexpr int kAgreeThreads = 256;
constexpr int kAgreeSlots = 4 * 6;             // (triplet type, location relation)

struct AgreeIds {
  int pid[6];                                  // __below__ __above__ __left of__ __right of__ __inside__ __surrounding__
};

__device__ __forceinline__ bool agrees_one(int slot, float4 sb, float4 ob, float2 sc, float2 oc, bool own_centres) {
  const float sx0 = clamp01(sb.x), sy0 = clamp01(sb.y), sw = clamp01(sb.z), sh = clamp01(sb.w);
  const float ox0 = clamp01(ob.x), oy0 = clamp01(ob.y), ow = clamp01(ob.z), oh = clamp01(ob.w);
  const float sxc = __fadd_rn(sx0, 0.5f * sw), syc = __fadd_rn(sy0, 0.5f * sh);
  const float oxc = __fadd_rn(ox0, 0.5f * ow), oyc = __fadd_rn(oy0, 0.5f * oh);
  const float scx = own_centres ? sc.x : sxc, scy = own_centres ? sc.y : syc;
  const float ocx = own_centres ? oc.x : oxc, ocy = own_centres ? oc.y : oyc;
  // a NaN anywhere in the pair: tested, never agreeing (the clamped values are finite or NaN: sxc is NaN iff x0 or w is)
  if (sxc != sxc || syc != syc || oxc != oxc || oyc != oyc || scx != scx || scy != scy || ocx != ocx || ocy != ocy) return false;
  const bool sur = sx0 < ox0 && sxc > oxc && sy0 < oy0 && syc > oyc;
  const bool ins = sx0 > ox0 && sxc < oxc && sy0 > oy0 && syc < oyc;
  if (slot == 5) return sur;
  if (slot == 4) return !sur && ins;
  if (sur || ins) return false;
  return slot == 3 ? scx > ocx : slot == 2 ? scx < ocx : slot == 0 ? scy > ocy : scy < ocy;
}

// one block per sample, lanes strided over the T rows.  per_sample[b][type] = {agreeing, tested};
// by_rel[b][type][relation] = {agreeing, tested} for the fold
__global__ __launch_bounds__(kAgreeThreads) void k_relation_agreement(
    const float4* __restrict__ boxes, const float2* __restrict__ centers, const int64_t* __restrict__ triplets,
    const int64_t* __restrict__ triplet_type, int O, int T, AgreeIds ids, uint8_t* __restrict__ tested,
    uint8_t* __restrict__ agrees, int64_t* __restrict__ per_sample, int64_t* __restrict__ by_rel) {
  __shared__ unsigned long long part[kAgreeThreads / 64][kAgreeSlots];
  const int b = blockIdx.x;
  const int64_t row = (int64_t)b * T, obj = (int64_t)b * O;
  unsigned long long acc[kAgreeSlots];
#pragma unroll
  for (int q = 0; q < kAgreeSlots; ++q) acc[q] = 0ull;
  for (int t = threadIdx.x; t < T; t += kAgreeThreads) {
    const int64_t* tr = triplets + (row + t) * 3;
    const int64_t s = tr[0], p = tr[1], o = tr[2], ty = triplet_type[row + t];
    int rel = -1;
#pragma unroll
    for (int r = 0; r < 6; ++r) rel = p == (int64_t)ids.pid[r] ? r : rel;
    const bool on = rel >= 0 && ty >= 0 && ty < 4 && s >= 0 && s < O && o >= 0 && o < O;
    bool ok = false;
    if (on) {
      const bool own = centers != nullptr;
      const float2 none = make_float2(0.f, 0.f);
      ok = agrees_one(rel, boxes[obj + s], boxes[obj + o], own ? centers[obj + s] : none, own ? centers[obj + o] : none, own);
    }
    tested[row + t] = on ? 1 : 0;
    agrees[row + t] = ok ? 1 : 0;
    const int slot = on ? (int)ty * 6 + rel : -1;
    const unsigned long long v = (ok ? (1ull << 32) : 0ull) | 1ull;
#pragma unroll
    for (int q = 0; q < kAgreeSlots; ++q) acc[q] += slot == q ? v : 0ull;      // no indexed register: no scratch
  }
#pragma unroll
  for (int q = 0; q < kAgreeSlots; ++q) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) acc[q] += __shfl_down(acc[q], off, 64);
  }
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  if (lane == 0) {
#pragma unroll
    for (int q = 0; q < kAgreeSlots; ++q) part[w][q] = acc[q];
  }
  __syncthreads();
  if (threadIdx.x < kAgreeSlots) {
    const int q = threadIdx.x;
    unsigned long long v = part[0][q];
    for (int k = 1; k < kAgreeThreads / 64; ++k) v += part[k][q];
    by_rel[((int64_t)b * kAgreeSlots + q) * 2 + 0] = (int64_t)(v >> 32);
    by_rel[((int64_t)b * kAgreeSlots + q) * 2 + 1] = (int64_t)(v & 0xffffffffull);
    part[0][q] = v;
  }
  __syncthreads();
  if (threadIdx.x < 4) {
    unsigned long long v = 0ull;
    for (int r = 0; r < 6; ++r) v += part[0][threadIdx.x * 6 + r];
    per_sample[((int64_t)b * 4 + threadIdx.x) * 2 + 0] = (int64_t)(v >> 32);
    per_sample[((int64_t)b * 4 + threadIdx.x) * 2 + 1] = (int64_t)(v & 0xffffffffull);
  }
}

// totals[type][pid[relation]][k] += sum_b by_rel[b][type][relation][k]: one wave per (type, relation), lanes strided over
// the samples, the same tree.  The six ids are distinct: no two blocks write one cell.
__global__ __launch_bounds__(64) void k_relation_agreement_fold(const int64_t* __restrict__ by_rel, int B, int P, AgreeIds ids,
                                                                int64_t* __restrict__ totals) {
  const int q = blockIdx.x, ty = q / 6, rel = q - ty * 6;
  int64_t a = 0, n = 0;
  for (int b = threadIdx.x; b < B; b += 64) {
    a += by_rel[((int64_t)b * kAgreeSlots + q) * 2 + 0];
    n += by_rel[((int64_t)b * kAgreeSlots + q) * 2 + 1];
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    a += __shfl_down(a, off, 64);
    n += __shfl_down(n, off, 64);
  }
  if (threadIdx.x == 0) {
    int pid = ids.pid[0];
#pragma unroll
    for (int r = 1; r < 6; ++r) pid = rel == r ? ids.pid[r] : pid;
    int64_t* cell = totals + ((int64_t)ty * P + pid) * 2;
    cell[0] = cell[0] + a;
    cell[1] = cell[1] + n;
  }
}

// ---- layout consistency: two layouts of the same objects (the robustness run: graph A against its rewritten graph B) -----
// Per counted object the IoU of the two clamped boxes (jaccard_one) and the L1 distance of their centres; per ordered pair
// (i, j) of counted objects the six verdicts of agrees_one on either layout.  One block per sample; both layouts are
// staged once in LDS (2 x O x 16 bytes, O <= 256: a thread stages one object and, as 16-byte rows read by consecutive
// lanes, conflict-free) and the lanes are strided over the O (O - 1) ordered pairs.  The counts are 20 integers per
// thread (a sample has at most 65 280 pairs): a shuffle tree per wave, then the waves in order through LDS; the four fp64
// sums through block_sum_f64.  No atomics: the same bits on every run.
constexpr int kConsThreads = 256;
constexpr int kConsCounts = 20;                // {in_a, in_b, in_both} x 6, same_pairs, pairs

__device__ __forceinline__ float4 clamp01_box(float4 v) { return make_float4(clamp01(v.x), clamp01(v.y), clamp01(v.z), clamp01(v.w)); }

// the six verdicts of one ordered pair as bits 0..5 (a NaN in the pair: none)
__device__ __forceinline__ unsigned verdicts(float4 sb, float4 ob) {
  const float2 none = make_float2(0.f, 0.f);
  unsigned m = 0u;
#pragma unroll
  for (int k = 0; k < 6; ++k) m |= agrees_one(k, sb, ob, none, none, false) ? (1u << k) : 0u;
  return m;
}

__global__ __launch_bounds__(kConsThreads) void k_layout_consistency(const float4* __restrict__ boxes_a,
                                                                    const float4* __restrict__ boxes_b,
                                                                    const uint8_t* __restrict__ counted, int O,
                                                                    float* __restrict__ iou_ab, float* __restrict__ shift,
                                                                    double* __restrict__ per_sample_f,
                                                                    int64_t* __restrict__ per_sample_i) {
  __shared__ float4 la[kConsThreads], lb[kConsThreads];
  __shared__ uint8_t lc[kConsThreads];
  __shared__ double fpart[kConsThreads / 64][4];
  __shared__ unsigned ipart[kConsThreads / 64][kConsCounts];
  const int b = blockIdx.x, o = threadIdx.x;
  const int64_t obj = (int64_t)b * O;
  double acc[4] = {0.0, 0.0, 0.0, 0.0};
  if (o < O) {                                   // O <= 256: one object per thread
    const float4 pa = boxes_a[obj + o], pb = boxes_b[obj + o];
    const bool on = counted[obj + o] != 0;
    la[o] = pa, lb[o] = pb, lc[o] = on ? 1 : 0;
    float v = 0.f, d = 0.f;
    if (on) {
      const float4 ca = clamp01_box(pa), cb = clamp01_box(pb);
      v = jaccard_one(ca, cb);                   // its own clamp of the first box changes nothing
      const float axc = __fadd_rn(ca.x, 0.5f * ca.z), ayc = __fadd_rn(ca.y, 0.5f * ca.w);
      const float bxc = __fadd_rn(cb.x, 0.5f * cb.z), byc = __fadd_rn(cb.y, 0.5f * cb.w);
      d = __fadd_rn(fabsf(__fsub_rn(axc, bxc)), fabsf(__fsub_rn(ayc, byc)));
      acc[0] = (double)v;
      acc[1] = v > 0.5f ? 1.0 : 0.0;
      acc[2] = (double)d;
      acc[3] = 1.0;
    }
    iou_ab[obj + o] = v;
    shift[obj + o] = d;
  }
  __syncthreads();
  unsigned cnt[kConsCounts];
#pragma unroll
  for (int q = 0; q < kConsCounts; ++q) cnt[q] = 0u;
  const int npairs = O * (O - 1);
  for (int q = threadIdx.x; q < npairs; q += kConsThreads) {
    const int i = q / (O - 1), r = q - i * (O - 1), j = r + (r >= i ? 1 : 0);
    if (lc[i] == 0 || lc[j] == 0) continue;
    const unsigned ma = verdicts(la[i], la[j]), mb = verdicts(lb[i], lb[j]);
#pragma unroll
    for (int k = 0; k < 6; ++k) {
      cnt[3 * k + 0] += (ma >> k) & 1u;
      cnt[3 * k + 1] += (mb >> k) & 1u;
      cnt[3 * k + 2] += ((ma & mb) >> k) & 1u;
    }
    cnt[18] += ma == mb ? 1u : 0u;
    cnt[19] += 1u;
  }
#pragma unroll
  for (int q = 0; q < kConsCounts; ++q) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) cnt[q] += __shfl_down(cnt[q], off, 64);
  }
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  if (lane == 0) {
#pragma unroll
    for (int q = 0; q < kConsCounts; ++q) ipart[w][q] = cnt[q];
  }
  block_sum_f64<4, kConsThreads / 64>(acc, fpart);        // its barrier publishes ipart as well
  if (threadIdx.x == 0) {
#pragma unroll
    for (int q = 0; q < 4; ++q) per_sample_f[(int64_t)b * 4 + q] = acc[q];
  }
  if (threadIdx.x < kConsCounts) {
    unsigned v = ipart[0][threadIdx.x];
    for (int k = 1; k < kConsThreads / 64; ++k) v += ipart[k][threadIdx.x];
    per_sample_i[(int64_t)b * kConsCounts + threadIdx.x] = (int64_t)v;
  }
}

// totals += the samples, in ascending sample order: thread q < 4 owns one fp64 sum, thread 4 + q one integer count
__global__ __launch_bounds__(64) void k_layout_consistency_fold(const double* __restrict__ per_sample_f,
                                                                const int64_t* __restrict__ per_sample_i, int B,
                                                                double* __restrict__ totals_f, int64_t* __restrict__ totals_i) {
  const int q = threadIdx.x;
  if (q < 4) {
    double v = totals_f[q];
    for (int b = 0; b < B; ++b) v += per_sample_f[(int64_t)b * 4 + q];
    totals_f[q] = v;
  } else if (q < 4 + kConsCounts) {
    int64_t v = totals_i[q - 4];
    for (int b = 0; b < B; ++b) v += per_sample_i[(int64_t)b * kConsCounts + q - 4];
    totals_i[q - 4] = v;
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

int64_t csg_relation_agreement_workspace(int64_t B) {
  if (B <= 0 || B > 65535) return 0;
  return B * kAgreeSlots * 2 * (int64_t)sizeof(int64_t);
}

int csg_relation_agreement(const float* boxes, const float* centers, const int64_t* triplets, const int64_t* triplet_type,
                           const int64_t* triplets_host, const int64_t* triplet_type_host, int64_t B, int64_t O, int64_t T,
                           int64_t P, const int32_t* pred_ids, uint8_t* tested, uint8_t* agrees, int64_t* per_sample,
                           int64_t* totals, void* workspace, int64_t workspace_bytes, void* stream) {
  CSG_REQUIRE(B > 0 && B <= 65535 && O > 0 && O <= (1 << 20) && T > 0 && T <= (1 << 20) && P > 0 && P <= 4096, CSG_E_BADSHAPE,
              "csg_relation_agreement: bad shape B=%ld O=%ld T=%ld P=%ld (B <= 65535, O <= 2^20, T <= 2^20, P <= 4096)",
              (long)B, (long)O, (long)T, (long)P);
  CSG_REQUIRE(boxes != nullptr && triplets != nullptr && triplet_type != nullptr && pred_ids != nullptr && tested != nullptr &&
                  agrees != nullptr && per_sample != nullptr && totals != nullptr && workspace != nullptr,
              CSG_E_BADSHAPE, "csg_relation_agreement: null operand");
  CSG_REQUIRE((triplets_host == nullptr) == (triplet_type_host == nullptr), CSG_E_BADSHAPE,
              "csg_relation_agreement: triplets_host and triplet_type_host come together or not at all");
  CSG_REQUIRE((uintptr_t)boxes % 16 == 0 && (uintptr_t)centers % 8 == 0 &&
                  ((uintptr_t)triplets | (uintptr_t)triplet_type | (uintptr_t)per_sample | (uintptr_t)totals |
                   (uintptr_t)workspace) % 8 == 0,
              CSG_E_BADSHAPE,
              "csg_relation_agreement: boxes must be 16-byte aligned, centers, the int64 operands and the workspace 8-byte aligned");
  CSG_REQUIRE(workspace_bytes >= csg_relation_agreement_workspace(B), CSG_E_WORKSPACE,
              "csg_relation_agreement: workspace of %ld bytes, %ld needed", (long)workspace_bytes,
              (long)csg_relation_agreement_workspace(B));
  AgreeIds ids;
  for (int a = 0; a < 8; ++a) {
    CSG_REQUIRE(pred_ids[a] >= 0 && pred_ids[a] < P, CSG_E_BADSHAPE,
                "csg_relation_agreement: predicate id %d outside [0, P = %ld)", (int)pred_ids[a], (long)P);
    for (int c = 0; c < a; ++c)
      CSG_REQUIRE(pred_ids[a] != pred_ids[c], CSG_E_BADSHAPE, "csg_relation_agreement: the eight predicate ids must be distinct");
    if (a >= 2) ids.pid[a - 2] = pred_ids[a];
  }
  if (triplets_host != nullptr) {                 // the rows' host copy: every tested row is checked before the first launch
    for (int64_t i = 0; i < B * T; ++i) {
      const int64_t s = triplets_host[i * 3], p = triplets_host[i * 3 + 1], o = triplets_host[i * 3 + 2];
      bool location = false;
      for (int r = 0; r < 6; ++r) location = location || p == (int64_t)ids.pid[r];
      if (!location) continue;
      CSG_REQUIRE(s >= 0 && s < O && o >= 0 && o < O, CSG_E_BADSHAPE,
                  "csg_relation_agreement: triplet %ld of sample %ld = (%ld, %ld, %ld) names an object outside [0, O = %ld)",
                  (long)(i % T), (long)(i / T), (long)s, (long)p, (long)o, (long)O);
      CSG_REQUIRE(triplet_type_host[i] >= 0 && triplet_type_host[i] < 4, CSG_E_BADSHAPE,
                  "csg_relation_agreement: triplet %ld of sample %ld has type %ld outside [0, 4)", (long)(i % T), (long)(i / T),
                  (long)triplet_type_host[i]);
    }
  }
  hipStream_t s = (hipStream_t)stream;
  CSG_LAUNCH(k_relation_agreement, dim3((unsigned)B), dim3(kAgreeThreads), 0, s, (const float4*)boxes, (const float2*)centers,
             triplets, triplet_type, (int)O, (int)T, ids, tested, agrees, per_sample, (int64_t*)workspace);
  CSG_LAUNCH(k_relation_agreement_fold, dim3(kAgreeSlots), dim3(64), 0, s, (const int64_t*)workspace, (int)B, (int)P, ids, totals);
  return check_launch("csg_relation_agreement");
}

int csg_layout_consistency(const float* boxes_a, const float* boxes_b, const uint8_t* counted, int64_t B, int64_t O,
                           float* iou_ab, float* shift, double* per_sample_f, int64_t* per_sample_i, double* totals_f,
                           int64_t* totals_i, void* stream) {
  CSG_REQUIRE(B > 0 && B <= 65535 && O > 0 && O <= kConsThreads, CSG_E_BADSHAPE,
              "csg_layout_consistency: bad shape B=%ld O=%ld (B <= 65535, O <= %d)", (long)B, (long)O, kConsThreads);
  CSG_REQUIRE(boxes_a != nullptr && boxes_b != nullptr && counted != nullptr && iou_ab != nullptr && shift != nullptr &&
                  per_sample_f != nullptr && per_sample_i != nullptr && totals_f != nullptr && totals_i != nullptr,
              CSG_E_BADSHAPE, "csg_layout_consistency: null operand");
  CSG_REQUIRE(((uintptr_t)boxes_a | (uintptr_t)boxes_b) % 16 == 0 &&
                  ((uintptr_t)per_sample_f | (uintptr_t)per_sample_i | (uintptr_t)totals_f | (uintptr_t)totals_i) % 8 == 0 &&
                  ((uintptr_t)iou_ab | (uintptr_t)shift) % 4 == 0,
              CSG_E_BADSHAPE,
              "csg_layout_consistency: boxes must be 16-byte aligned, the fp64 and int64 outputs 8-byte, the fp32 outputs 4-byte");
  hipStream_t s = (hipStream_t)stream;
  CSG_LAUNCH(k_layout_consistency, dim3((unsigned)B), dim3(kConsThreads), 0, s, (const float4*)boxes_a, (const float4*)boxes_b,
             counted, (int)O, iou_ab, shift, per_sample_f, per_sample_i);
  CSG_LAUNCH(k_layout_consistency_fold, dim3(1), dim3(64), 0, s, (const double*)per_sample_f, (const int64_t*)per_sample_i, (int)B,
             totals_f, totals_i);
  return check_launch("csg_layout_consistency");
}

}  // extern "C"
