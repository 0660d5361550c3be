// COCO segmentations -> per-object M x M masks and mask centroids: what the reference's COCO __getitem__ does per object
// through pycocotools and OpenCV (sg2im/data/packed_coco.py:305-351, sg2im/data/coco.py:317-363), for a padded batch, one
// block per (sample, object) row.
//
// The reference decodes the whole HH x WW mask (seg_to_mask), crops it to the rounded box, resizes the crop to M x M with
// cv2.INTER_NEAREST and takes the centroid of the result on torch.linspace(x0, x0 + w, M).  Nearest-neighbour resizing reads
// M source columns and M source rows of the picture and nothing else, so only those M x M pixels are evaluated here; the
// full-resolution mask is never made.
//
//   source index   sx[c] = crop.x0 + min(floor(c * ifx), cw - 1), ifx = 1.0 / ((double) M / cw) — cv2's own expression with its
//                  two roundings, not cw / M; rows likewise.
//   polygons       pycocotools' rleFrPoly at scale 5: vertices (int)(5 x + .5), every edge walked one grid step at a time,
//                  (u, v) = (t + xs, (int)(ys + s t + .5)) for dx >= dy and ((int)(xs + s t + .5), t + ys) otherwise, and a toggle
//                  wherever u steps across the middle of a pixel column: between u = 5 X + 2 and 5 X + 3 for column X, at row
//                  yd = ceil(clamp((min(v) + .5) / 5 - .5, 0, HH)).  A column's crossings are even in number, so a pixel's value
//                  is the parity of the crossings of ITS column with yd <= y.  Along an edge u is monotone in t, so an edge
//                  crosses a level at most once: directly at t = U - xs for dx >= dy, by bisection on t for dx < dy — the same
//                  fp64 expressions, operation by operation (compiled with -ffp-contract=off), so the same integers.
//                  Threads run over (needed column, edge) pairs and toggle an LDS cell (column, first needed row with
//                  sy >= yd); a prefix parity runs down each column; the polygons of an object are ORed (merge is a union).
//   runs           pixel (x, y) is parity(#{toggles <= x * HH + y}), the toggles being the running sums of the run lengths: one
//                  binary search per output pixel.
//   centre         count, sum of columns and sum of rows of the M x M mask as integers, then in fp64
//                  x0 + ((fp32)(x0 + w) - x0) * sum_col / ((M - 1) * count), rounded once to fp32; x0 + 0.5 w in fp32 for an empty
//                  mask (the reference's fallback, and the collate's box centre).
// Only integer LDS atomics (parities: the order cannot matter) and an ordered integer reduction: the same bytes on every run.
#include "csg_common.h"

namespace csg {

constexpr int kMaskThreads = 256;
constexpr int kMaskMaxM = CSG_COCO_MASKS_MAX_M;
constexpr double kMaskMaxCoord = CSG_COCO_MASKS_MAX_COORD;

__device__ __forceinline__ int grid_coord(double x) {
  x = fmin(fmax(x, -kMaskMaxCoord), kMaskMaxCoord);      // the host refused anything beyond; a stale buffer stays in range
  return (int)(5.0 * x + .5);
}

__device__ __forceinline__ int u_at(int xs, double s, int t) { return (int)(xs + s * t + .5); }

// The row yd at which the edge (xs, ys) -> (xe, ye) toggles the pixel column whose level lies between u = U and U + 1, or -1.
__device__ __forceinline__ int edge_crossing(int xs, int ys, int xe, int ye, int U, int HH) {
  const int dx = abs(xe - xs), dy = abs(ys - ye);
  if ((dx >= dy && xs > xe) || (dx < dy && ys > ye)) {
    int t = xs; xs = xe; xe = t;
    t = ys; ys = ye; ye = t;
  }
  int mv;
  if (dx >= dy) {
    if (!(xs <= U && U < xe)) return -1;
    const double s = (double)(ye - ys) / dx;
    const int t0 = U - xs;
    const int v0 = (int)(ys + s * t0 + .5), v1 = (int)(ys + s * (t0 + 1) + .5);
    mv = min(v0, v1);
  } else {
    const double s = (double)(xe - xs) / dy;
    if (s == 0.0) return -1;
    const bool up = s > 0.0;
    const int u0 = u_at(xs, s, 0), u1 = u_at(xs, s, dy);
    if (up ? (u0 >= U + 1 || u1 < U + 1) : (u0 <= U || u1 > U)) return -1;
    int lo = 0, hi = dy;                                   // not yet across at lo, across at hi
    while (hi - lo > 1) {
      const int mid = lo + ((hi - lo) >> 1);
      const int u = u_at(xs, s, mid);
      if (up ? u >= U + 1 : u <= U) hi = mid; else lo = mid;
    }
    mv = ys + hi - 1;
  }
  double yd = ((double)mv + .5) / 5.0 - .5;
  yd = yd < 0.0 ? 0.0 : (yd > (double)HH ? (double)HH : yd);
  return (int)ceil(yd);
}

__global__ __launch_bounds__(kMaskThreads) void k_coco_masks(
    const uint8_t* __restrict__ kind, const int32_t* __restrict__ crop, const int64_t* __restrict__ sizes,
    const float4* __restrict__ boxes, const int32_t* __restrict__ obj_poly, const int32_t* __restrict__ poly_off,
    const double* __restrict__ poly_xy, const int32_t* __restrict__ obj_runs, const int32_t* __restrict__ toggles, int O, int P,
    int V, int T, int M, int64_t* __restrict__ masks, float2* __restrict__ centers) {
  __shared__ int cells[kMaskMaxM * (kMaskMaxM + 1)];
  __shared__ unsigned char acc[kMaskMaxM * kMaskMaxM];
  __shared__ int sx[kMaskMaxM], sy[kMaskMaxM];
  __shared__ int part[kMaskThreads / 64][3];
  const int tid = threadIdx.x;
  const int row = blockIdx.x;                              // b * (O + 1) + o
  const int b = row / (O + 1), o = row - b * (O + 1);
  const int MM = M * M;
  int64_t* out = masks == nullptr ? nullptr : masks + (int64_t)row * MM;
  if (o == O) {                                            // the __image__ row the collate appends: all ones
    if (out != nullptr)
      for (int i = tid; i < MM; i += kMaskThreads) out[i] = 1;
    return;
  }
  const int obj = b * O + o;
  const int what = kind[obj];
  const int64_t HH64 = sizes[2 * b], WW64 = sizes[2 * b + 1];
  const int cx0 = crop[4 * obj], cy0 = crop[4 * obj + 1], cx1 = crop[4 * obj + 2], cy1 = crop[4 * obj + 3];
  // every condition below is uniform over the block.  The host refused what fails them; a device row that disagrees with its
  // host copy (a stale buffer under a replayed graph) becomes a padding row, and nothing is indexed with it.
  const bool live = (what == 1 || what == 2) && HH64 >= 1 && WW64 >= 1 && HH64 <= CSG_COCO_MASKS_MAX_SIDE &&
                    WW64 <= CSG_COCO_MASKS_MAX_SIDE && HH64 * WW64 <= (int64_t)INT32_MAX && cx0 >= 0 && cx0 < cx1 && (int64_t)cx1 <= WW64 && cy0 >= 0 &&
                    cy0 < cy1 && (int64_t)cy1 <= HH64;
  const int HH = (int)HH64;
  for (int i = tid; i < MM; i += kMaskThreads) acc[i] = 0;
  if (live && tid < M) {
    const int cw = cx1 - cx0, ch = cy1 - cy0;
    const double ifx = 1.0 / ((double)M / (double)cw), ify = 1.0 / ((double)M / (double)ch);
    sx[tid] = cx0 + min((int)floor((double)tid * ifx), cw - 1);
    sy[tid] = cy0 + min((int)floor((double)tid * ify), ch - 1);
  }
  __syncthreads();
  if (live && what == 1) {
    const int64_t first = obj_poly[2 * obj], count = obj_poly[2 * obj + 1];
    if (first >= 0 && count >= 0 && first + count <= (int64_t)P) {
      for (int p = (int)first; p < (int)(first + count); ++p) {
        const int v0 = poly_off[p], v1 = poly_off[p + 1];
        const int k = v1 - v0;
        if (v0 < 0 || v1 > V || k < 1) continue;
        for (int i = tid; i < M * (M + 1); i += kMaskThreads) cells[i] = 0;
        __syncthreads();
        const double* xy = poly_xy + 2 * (int64_t)v0;
        for (int idx = tid; idx < k * M; idx += kMaskThreads) {
          const int e = idx / M, c = idx - e * M;
          const int e1 = e + 1 == k ? 0 : e + 1;
          const int yd = edge_crossing(grid_coord(xy[2 * e]), grid_coord(xy[2 * e + 1]), grid_coord(xy[2 * e1]),
                                       grid_coord(xy[2 * e1 + 1]), 5 * sx[c] + 2, HH);
          if (yd < 0) continue;
          int lo = 0, hi = M;                              // the first needed row with sy >= yd; M: below all of them
          while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (sy[mid] >= yd) hi = mid; else lo = mid + 1;
          }
          atomicXor(&cells[c * (M + 1) + lo], 1);
        }
        __syncthreads();
        if (tid < M) {
          int par = 0;
          for (int r = 0; r < M; ++r) {
            par ^= cells[tid * (M + 1) + r];
            if (par) acc[r * M + tid] = 1;
          }
        }
        __syncthreads();
      }
    }
  } else if (live && what == 2) {
    const int64_t first = obj_runs[2 * obj], count = obj_runs[2 * obj + 1];
    if (first >= 0 && count >= 0 && first + count <= (int64_t)T) {
      const int32_t* tg = toggles + first;
      for (int i = tid; i < MM; i += kMaskThreads) {
        const int r = i / M, c = i - r * M;
        const int64_t at = (int64_t)sx[c] * HH + sy[r];
        int lo = 0, hi = (int)count;                       // the number of toggles <= at
        while (lo < hi) {
          const int mid = lo + ((hi - lo) >> 1);
          if ((int64_t)tg[mid] <= at) lo = mid + 1; else hi = mid;
        }
        acc[i] = (unsigned char)(lo & 1);
      }
    }
  }
  __syncthreads();
  int v[3] = {0, 0, 0};                                    // count, sum of columns, sum of rows: at most 64 * 64 * 63
  for (int i = tid; i < MM; i += kMaskThreads) {
    const int bit = acc[i];
    const int r = i / M;
    if (out != nullptr) out[i] = bit;
    v[0] += bit;
    v[1] += bit * (i - r * M);
    v[2] += bit * r;
  }
#pragma unroll
  for (int q = 0; q < 3; ++q) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v[q] += __shfl_down(v[q], off, 64);
  }
  if ((tid & 63) == 0) {
#pragma unroll
    for (int q = 0; q < 3; ++q) part[tid >> 6][q] = v[q];
  }
  __syncthreads();
  if (tid == 0) {
    for (int w = 1; w < kMaskThreads / 64; ++w) {
#pragma unroll
      for (int q = 0; q < 3; ++q) v[q] += part[w][q];
    }
    const float4 bx = boxes[obj];
    float2 c;
    if (v[0] == 0) {
      c = make_float2(bx.x + 0.5f * bx.z, bx.y + 0.5f * bx.w);
    } else {
      const double den = (double)((M - 1) * v[0]);
      const float hx = bx.x + bx.z, hy = bx.y + bx.w;
      c = make_float2((float)((double)bx.x + (((double)hx - (double)bx.x) * (double)v[1]) / den),
                      (float)((double)bx.y + (((double)hy - (double)bx.y) * (double)v[2]) / den));
    }
    centers[obj] = c;
  }
}

}  // namespace csg

using namespace csg;

extern "C" {

int csg_coco_masks(const uint8_t* kind, const int32_t* crop, const int64_t* sizes, const float* boxes, const int32_t* obj_poly,
                   const int32_t* poly_off, const double* poly_xy, const int32_t* obj_runs, const int32_t* toggles,
                   const uint8_t* kind_host, const int32_t* crop_host, const int64_t* sizes_host, const int32_t* obj_poly_host,
                   const int32_t* poly_off_host, const double* poly_xy_host, const int32_t* obj_runs_host, int64_t B, int64_t O,
                   int64_t P, int64_t V, int64_t T, int64_t M, int64_t* masks, float* centers, void* stream) {
  CSG_REQUIRE(M >= 2 && M <= CSG_COCO_MASKS_MAX_M && (M & (M - 1)) == 0, CSG_E_UNSUPPORTED,
              "csg_coco_masks: mask size M = %ld, a power of two in 2 .. %d", (long)M, CSG_COCO_MASKS_MAX_M);
  CSG_REQUIRE(B >= 1 && B <= CSG_COCO_MASKS_MAX_BATCH && O >= 1 && O <= CSG_COCO_MASKS_MAX_OBJECTS, CSG_E_BADSHAPE,
              "csg_coco_masks: bad shape B=%ld O=%ld (1 <= B <= %d, 1 <= O <= %d)", (long)B, (long)O, CSG_COCO_MASKS_MAX_BATCH,
              CSG_COCO_MASKS_MAX_OBJECTS);
  CSG_REQUIRE(P >= 0 && V >= 0 && T >= 0 && P <= CSG_COCO_MASKS_MAX_VERTICES && V <= CSG_COCO_MASKS_MAX_VERTICES &&
                  T <= INT32_MAX,
              CSG_E_BADSHAPE, "csg_coco_masks: P=%ld polygons, V=%ld vertices (at most %d each), T=%ld toggles (below 2^31)",
              (long)P, (long)V, CSG_COCO_MASKS_MAX_VERTICES, (long)T);
  CSG_REQUIRE(kind != nullptr && crop != nullptr && sizes != nullptr && boxes != nullptr && obj_poly != nullptr &&
                  poly_off != nullptr && obj_runs != nullptr && kind_host != nullptr && crop_host != nullptr &&
                  sizes_host != nullptr && obj_poly_host != nullptr && poly_off_host != nullptr && obj_runs_host != nullptr &&
                  centers != nullptr && (V == 0 || (poly_xy != nullptr && poly_xy_host != nullptr)) &&
                  (T == 0 || toggles != nullptr),
              CSG_E_BADSHAPE, "csg_coco_masks: null operand");
  CSG_REQUIRE(((uintptr_t)boxes & 15) == 0 &&
                  (((uintptr_t)sizes | (uintptr_t)masks | (uintptr_t)centers | (uintptr_t)poly_xy) & 7) == 0 &&
                  (((uintptr_t)crop | (uintptr_t)obj_poly | (uintptr_t)poly_off | (uintptr_t)obj_runs | (uintptr_t)toggles) & 3) == 0,
              CSG_E_BADSHAPE,
              "csg_coco_masks: boxes must be 16-byte aligned, sizes / masks / centers / poly_xy 8-byte, the int32 operands 4-byte");
  CSG_REQUIRE(poly_off_host[0] >= 0 && (int64_t)poly_off_host[P] <= V, CSG_E_BADSHAPE,
              "csg_coco_masks: poly_off runs from %d to %d, inside [0, V = %ld]", (int)poly_off_host[0], (int)poly_off_host[P],
              (long)V);
  for (int64_t p = 0; p < P; ++p)
    CSG_REQUIRE(poly_off_host[p] <= poly_off_host[p + 1], CSG_E_BADSHAPE, "csg_coco_masks: poly_off decreases at polygon %ld",
                (long)p);
  for (int64_t i = 0; i < 2 * V; ++i)
    CSG_REQUIRE(poly_xy_host[i] >= -CSG_COCO_MASKS_MAX_COORD && poly_xy_host[i] <= CSG_COCO_MASKS_MAX_COORD, CSG_E_BADSHAPE,
                "csg_coco_masks: polygon coordinate %ld is %g, within +-%g", (long)i, poly_xy_host[i],
                (double)CSG_COCO_MASKS_MAX_COORD);
  for (int64_t b = 0; b < B; ++b) {
    const int64_t HH = sizes_host[2 * b], WW = sizes_host[2 * b + 1];
    CSG_REQUIRE(HH >= 1 && WW >= 1 && HH <= CSG_COCO_MASKS_MAX_SIDE && WW <= CSG_COCO_MASKS_MAX_SIDE &&
                    HH * WW <= (int64_t)INT32_MAX,
                CSG_E_BADSHAPE,
                "csg_coco_masks: the picture of sample %ld is %ld x %ld (HH x WW), 1 .. %d on a side and fewer than 2^31 pixels",
                (long)b, (long)HH, (long)WW, CSG_COCO_MASKS_MAX_SIDE);
    for (int64_t o = 0; o < O; ++o) {
      const int64_t i = b * O + o;
      const int what = kind_host[i];
      CSG_REQUIRE(what >= 0 && what <= 2, CSG_E_BADSHAPE,
                  "csg_coco_masks: sample %ld object %ld: kind = %d, 0 (padding), 1 (polygons) or 2 (runs)", (long)b, (long)o, what);
      if (what == 0) continue;
      const int32_t* c = crop_host + 4 * i;
      CSG_REQUIRE(c[0] >= 0 && c[0] < c[2] && (int64_t)c[2] <= WW && c[1] >= 0 && c[1] < c[3] && (int64_t)c[3] <= HH,
                  CSG_E_BADSHAPE,
                  "csg_coco_masks: sample %ld object %ld: crop (%d, %d, %d, %d) is empty or outside the %ld x %ld picture (WW x HH)",
                  (long)b, (long)o, (int)c[0], (int)c[1], (int)c[2], (int)c[3], (long)WW, (long)HH);
      const int32_t* r = (what == 1 ? obj_poly_host : obj_runs_host) + 2 * i;
      const int64_t lim = what == 1 ? P : T;
      CSG_REQUIRE(r[0] >= 0 && r[1] >= 0 && (int64_t)r[0] + r[1] <= lim, CSG_E_BADSHAPE,
                  "csg_coco_masks: sample %ld object %ld: %s %d .. %d + %d, inside [0, %ld]", (long)b, (long)o,
                  what == 1 ? "polygons" : "toggles", (int)r[0], (int)r[0], (int)r[1], (long)lim);
    }
  }
  hipStream_t s = (hipStream_t)stream;
  ProfScope p(K_COCO_MASKS, (double)B * (O + 1) * M * M * 8 + (double)V * 16 + (double)T * 4, s);
  CSG_LAUNCH(k_coco_masks, dim3((unsigned)(B * (O + 1))), dim3(kMaskThreads), 0, s, kind, crop, sizes, (const float4*)boxes,
             obj_poly, poly_off, poly_xy, obj_runs, toggles, (int)O, (int)P, (int)V, (int)T, (int)M, masks, (float2*)centers);
  return check_launch("csg_coco_masks");
}

}  // extern "C"
