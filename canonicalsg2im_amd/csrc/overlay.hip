// Box outlines on a uint8 picture: the layout picture of the reference's scripts/run_model.py (img_%06d_layout.png:
// the generated image with the predicted boxes on it, sg2im/vis.py:128-146), without matplotlib; the boxes' text labels are
// a launch of their own on the outlined picture, csg_draw_labels_u8 below; the picture of the scene graph itself
// (img_%06d_sg.png) is csg_draw_graph_u8, last in this file.
// The rule is defined to the byte and restated in numpy by tests/overlay_cases.py:
//   row o of sample b is SKIPPED when objs[b,o,0] == image_id, or all four box values are -1, or one of them is NaN, or
//   w <= 0 or h <= 0;  otherwise, in fp32 and in this order (this file is compiled with -ffp-contract=off):
//     x0 = clamp(x, 0, 1), x1 = clamp(x + w, 0, 1)                        (y likewise; clamp of a NaN sum is 0)
//     px0 = min(W - 1, (int)(x0 * W)), px1 = max(px0, min(W - 1, (int)(x1 * W) - 1))   (y likewise with H)
//   a pixel is on the outline of o when it lies in [px0, px1] x [py0, py1] and its distance to the nearest side of that
//   rectangle is < thickness;  it takes palette[o % P] of the HIGHEST such o, or keeps its byte.
// Every lane decides its own four pixels by scanning the sample's rows from the highest down: no two lanes write the same
// byte, nothing is accumulated, the result is the same on every run.  One launch, nothing read back.
#include "csg_common.h"

namespace csg {

constexpr int kOverlayMaxRows = 256;      // objects per sample, __image__ and padding included (as csg_canon_general_*)
constexpr int kOverlayMaxColours = 256;

__device__ __forceinline__ float clamp01(float v) { return v > 0.f ? (v < 1.f ? v : 1.f) : 0.f; }

// (px0, py0, px1, py1) of row `row` = b * O + o, or px0 < 0 for a row that is not drawn: the one statement of the pixel
// rule's fp32 part, read by the outline kernel and by the label kernel
__device__ __forceinline__ int4 pixel_rect(const float* __restrict__ boxes, const int64_t* __restrict__ objs, int64_t row, int A,
                                           int H, int W, int64_t image_id) {
  const float4 q = *(const float4*)(boxes + row * 4);
  const bool pad = q.x == -1.f && q.y == -1.f && q.z == -1.f && q.w == -1.f;
  const bool nan = q.x != q.x || q.y != q.y || q.z != q.z || q.w != q.w;
  int4 r = make_int4(-1, -1, -1, -1);
  if (objs[row * A] != image_id && !pad && !nan && q.z > 0.f && q.w > 0.f) {
    const float x0 = clamp01(q.x), x1 = clamp01(q.x + q.z);
    const float y0 = clamp01(q.y), y1 = clamp01(q.y + q.w);
    r.x = min(W - 1, (int)(x0 * (float)W));
    r.z = max(r.x, min(W - 1, (int)(x1 * (float)W) - 1));
    r.y = min(H - 1, (int)(y0 * (float)H));
    r.w = max(r.y, min(H - 1, (int)(y1 * (float)H) - 1));
  }
  return r;
}

// out (B,3,H,W) uint8 planar, W % 4 == 0: a lane owns four consecutive pixels of one row and writes one dword per plane,
// so a wave stores 256 contiguous bytes per plane
__global__ __launch_bounds__(256) void k_draw_boxes_u8(const uint8_t* __restrict__ img, const float* __restrict__ boxes,
                                                        const int64_t* __restrict__ objs, int O, int A, int H, int W,
                                                        int64_t image_id, const uint8_t* __restrict__ palette, int P,
                                                        int thickness, uint8_t* __restrict__ out) {
  __shared__ int4 s_rect[kOverlayMaxRows];          // px0, py0, px1, py1; px0 < 0: skipped
  __shared__ uint32_t s_rgb[kOverlayMaxColours];
  const int b = blockIdx.y, tid = threadIdx.x;
  for (int o = tid; o < O; o += 256) s_rect[o] = pixel_rect(boxes, objs, (int64_t)b * O + o, A, H, W, image_id);
  for (int p = tid; p < P; p += 256)
    s_rgb[p] = (uint32_t)palette[p * 3] | (uint32_t)palette[p * 3 + 1] << 8 | (uint32_t)palette[p * 3 + 2] << 16;
  __syncthreads();
  const int64_t npix = (int64_t)H * W, nquad = npix >> 2;
  const uint8_t* ib = img + (int64_t)b * 3 * npix;
  uint8_t* ob = out + (int64_t)b * 3 * npix;
  for (int64_t q = (int64_t)blockIdx.x * 256 + tid; q < nquad; q += (int64_t)gridDim.x * 256) {
    const int y = (int)((q * 4) / W), x = (int)((q * 4) % W);
    int win[4] = {-1, -1, -1, -1};
    int open = 4;
    for (int o = O - 1; o >= 0 && open; --o) {      // the LDS reads are wave-uniform (one broadcast each)
      const int4 r = s_rect[o];
      if (r.x < 0 || y < r.y || y > r.w) continue;
      const int dy = min(y - r.y, r.w - y);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int xx = x + j;
        if (win[j] >= 0 || xx < r.x || xx > r.z) continue;
        if (min(dy, min(xx - r.x, r.z - xx)) < thickness) {
          win[j] = o;
          --open;
        }
      }
    }
    uint32_t word[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) word[c] = *(const uint32_t*)(ib + (int64_t)c * npix + q * 4);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (win[j] < 0) continue;
      const uint32_t rgb = s_rgb[win[j] % P];
#pragma unroll
      for (int c = 0; c < 3; ++c) word[c] = (word[c] & ~(0xffu << (8 * j))) | ((rgb >> (8 * c)) & 0xffu) << (8 * j);
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) *(uint32_t*)(ob + (int64_t)c * npix + q * 4) = word[c];
  }
}

// ---- the boxes' names (csg_draw_labels_u8) --------------------------------------------------------------------------
// A strip of at most nine lines across the top of each box, blended half and half with palette[o % P], with the label in a
// 5 x 7 font on its lines 1..7 (include/csg_hip.h states the rule; tests/label_cases.py restates it in numpy).  The same
// walk as the outlines: a lane owns four pixels of one line, the highest row whose strip holds a pixel decides it.
constexpr int kFontRows = 7;
constexpr int kFontBytes = 95 * kFontRows;          // glyphs of the bytes 32 .. 126
constexpr int kFontUnknown = '?' - 32;

__global__ __launch_bounds__(256) void k_draw_labels_u8(const uint8_t* __restrict__ img, const float* __restrict__ boxes,
                                                         const int64_t* __restrict__ objs, int O, int A, int H, int W,
                                                         int64_t image_id, const uint8_t* __restrict__ palette, int P,
                                                         const uint8_t* __restrict__ text, const int32_t* __restrict__ text_off,
                                                         const uint8_t* __restrict__ font, uint8_t* __restrict__ out) {
  __shared__ int4 s_strip[kOverlayMaxRows];         // px0, py0, px1, the strip's last line; px0 < 0: no strip
  __shared__ int4 s_label[kOverlayMaxRows];         // the label's first byte in `text`, its bytes n, tx
  __shared__ uint32_t s_rgb[kOverlayMaxColours];
  __shared__ uint8_t s_font[(kFontBytes + 3) & ~3];
  const int b = blockIdx.y, tid = threadIdx.x;
  for (int o = tid; o < O; o += 256) {
    const int64_t row = (int64_t)b * O + o;
    int4 r = pixel_rect(boxes, objs, row, A, H, W, image_id);
    const int first = text_off[row], n = text_off[row + 1] - first;
    int4 l = make_int4(first, n, 0, 0);
    if (first < 0 || n <= 0) r.x = -1;              // no label: no strip either
    if (r.x >= 0) {
      r.w = min(r.w, r.y + 8);
      const int64_t slack = (int64_t)(r.z - r.x + 1) - (6ll * n - 1);           // rw - tw
      l.z = r.x + (slack > 0 ? (int)(slack / 2) : 0);
    }
    s_strip[o] = r;
    s_label[o] = l;
  }
  for (int p = tid; p < P; p += 256)
    s_rgb[p] = (uint32_t)palette[p * 3] | (uint32_t)palette[p * 3 + 1] << 8 | (uint32_t)palette[p * 3 + 2] << 16;
  for (int i = tid; i < kFontBytes; i += 256) s_font[i] = font[i];
  __syncthreads();
  const int64_t npix = (int64_t)H * W, nquad = npix >> 2;
  const uint8_t* ib = img + (int64_t)b * 3 * npix;
  uint8_t* ob = out + (int64_t)b * 3 * npix;
  for (int64_t q = (int64_t)blockIdx.x * 256 + tid; q < nquad; q += (int64_t)gridDim.x * 256) {
    const int y = (int)((q * 4) / W), x = (int)((q * 4) % W);
    int win[4] = {-1, -1, -1, -1};
    int open = 4;
    for (int o = O - 1; o >= 0 && open; --o) {      // the LDS reads are wave-uniform (one broadcast each)
      const int4 r = s_strip[o];
      if (r.x < 0 || y < r.y || y > r.w) continue;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int xx = x + j;
        if (win[j] >= 0 || xx < r.x || xx > r.z) continue;
        win[j] = o;
        --open;
      }
    }
    uint32_t word[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) word[c] = *(const uint32_t*)(ib + (int64_t)c * npix + q * 4);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (win[j] < 0) continue;
      const int4 r = s_strip[win[j]], l = s_label[win[j]];
      const int line = y - r.y - 1, col = x + j - l.z;
      bool ink = false;
      if (line >= 0 && line < kFontRows && col >= 0) {
        const int k = col / 6, bit = col - 6 * k;   // k < n and bit < 5  <=>  col < tw = 6 n - 1 and col % 6 < 5
        if (k < l.y && bit < 5) {
          const int byte = text[l.x + k];
          const int g = byte >= 32 && byte <= 126 ? byte - 32 : kFontUnknown;
          ink = (s_font[g * kFontRows + line] >> (4 - bit)) & 1;
        }
      }
      const uint32_t rgb = s_rgb[win[j] % P];
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const uint32_t half = (((word[c] >> (8 * j)) & 0xffu) + ((rgb >> (8 * c)) & 0xffu) + 1u) >> 1;
        word[c] = (word[c] & ~(0xffu << (8 * j))) | (ink ? 0u : half) << (8 * j);
      }
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) *(uint32_t*)(ob + (int64_t)c * npix + q * 4) = word[c];
  }
}

// ---- scene-graph pictures (csg_draw_graph_u8) ----------------------------------------------------------------------
// A batch of canvases painted from per-picture lists of primitives: segments, triangles (arrowheads) and labelled nodes
// (include/csg_hip.h states the record and the pixel rule; tests/sgdraw_cases.py restates the rule in numpy).  All
// geometry is integer: no floating point below.  A block owns a 64 x 16 tile of one canvas, a lane four consecutive
// pixels of one of its lines.  Per pass the block takes 256 consecutive records of its picture, the highest first, keeps
// those whose bounding box meets the tile (ballot + prefix popcount: the list stays in record order, highest first, and
// with one candidate per thread it cannot overflow), and every lane scans the list until its four pixels are decided.
// The passes end when the records do, or when every pixel of the tile is decided.
constexpr int kGraphList = 256;           // records per pass = the list's capacity = the block's threads
constexpr int kGraphTileW = 64, kGraphTileH = 16;
constexpr int kGraphSegment = 0, kGraphTriangle = 1, kGraphNode = 2;

__device__ __forceinline__ int64_t cross64(int ax, int ay, int bx, int by) { return (int64_t)ax * by - (int64_t)ay * bx; }

// does record (a, c) cover pixel (x, y), and is the pixel label ink?  The one statement of the pixel rule.
__device__ __forceinline__ bool graph_covers(const int4 a, const int4 c, int x, int y, const uint8_t* __restrict__ text,
                                             int64_t text_bytes, const uint8_t* s_font, bool& ink) {
  const int kind = a.x & 15, param = (a.x >> 4) & 15;
  ink = false;
  if (kind == kGraphSegment) {
    const int64_t dx = (int64_t)a.w - a.y, dy = (int64_t)c.x - a.z, vx = (int64_t)x - a.y, vy = (int64_t)y - a.z;
    const int64_t L2 = dx * dx + dy * dy, dot = vx * dx + vy * dy, t2 = (int64_t)param * param;
    if (L2 == 0 || dot <= 0) return 4 * (vx * vx + vy * vy) <= t2;
    if (dot >= L2) {
      const int64_t wx = (int64_t)x - a.w, wy = (int64_t)y - c.x;
      return 4 * (wx * wx + wy * wy) <= t2;
    }
    const int64_t cr = vx * dy - vy * dx;
    return 4 * cr * cr <= t2 * L2;
  }
  if (kind == kGraphTriangle) {
    const int x0 = a.y, y0 = a.z, x1 = a.w, y1 = c.x, x2 = c.y, y2 = c.z;
    if (cross64(x1 - x0, y1 - y0, x2 - x0, y2 - y0) == 0) return false;
    const int64_t e0 = cross64(x1 - x0, y1 - y0, x - x0, y - y0), e1 = cross64(x2 - x1, y2 - y1, x - x1, y - y1),
                  e2 = cross64(x0 - x2, y0 - y2, x - x2, y - y2);
    return (e0 >= 0 && e1 >= 0 && e2 >= 0) || (e0 <= 0 && e1 <= 0 && e2 <= 0);
  }
  if (kind != kGraphNode) return false;
  const int x0 = a.y, y0 = a.z, x1 = a.w, y1 = c.x;
  if (x < x0 || x > x1 || y < y0 || y > y1) return false;
  const int re = min(param, min((x1 - x0) / 2, (y1 - y0) / 2));
  const int cx = x < x0 + re ? x0 + re - x : (x > x1 - re ? x - (x1 - re) : 0);
  const int cy = y < y0 + re ? y0 + re - y : (y > y1 - re ? y - (y1 - re) : 0);
  if (cx > 0 && cy > 0 && cx * cx + cy * cy > re * re) return false;
  const int64_t first = c.y, n = c.z;
  const int64_t wslack = (int64_t)(x1 - x0 + 1) - (6 * n - 1), hslack = (int64_t)(y1 - y0 + 1) - kFontRows;
  const int64_t col = (int64_t)x - (x0 + (wslack > 0 ? wslack / 2 : 0));
  const int line = y - (y0 + (hslack > 0 ? (int)(hslack / 2) : 0));
  if (line >= 0 && line < kFontRows && col >= 0) {
    const int64_t k = col / 6;                       // k < n and bit < 5  <=>  col < tw = 6 n - 1 and col % 6 < 5
    const int bit = (int)(col - 6 * k);
    if (k < n && bit < 5) {
      // a label range outside the text is refused where the records are built; here it only draws '?'
      const int byte = first >= 0 && first + k < text_bytes ? text[first + k] : 0;
      const int g = byte >= 32 && byte <= 126 ? byte - 32 : kFontUnknown;
      ink = (s_font[g * kFontRows + line] >> (4 - bit)) & 1;
    }
  }
  return true;
}

// out (B,3,H,W) uint8 planar, W % 4 == 0; grid (cdiv(W, 64), cdiv(H, 16), B); every byte of out is written
__global__ __launch_bounds__(256) void k_draw_graph_u8(const int4* __restrict__ prims, int n_prims,
                                                        const int32_t* __restrict__ prim_off,
                                                        const uint8_t* __restrict__ text, int64_t text_bytes,
                                                        const uint8_t* __restrict__ font, int H, int W, uint32_t background,
                                                        uint8_t* __restrict__ out) {
  __shared__ int4 s_rec[kGraphList * 2];             // the pass's records that meet the tile, the highest first
  __shared__ int4 s_box[kGraphList];                 // their bounding boxes x0, y0, x1, y1 (a segment's inflated by t)
  __shared__ uint8_t s_font[(kFontBytes + 3) & ~3];
  __shared__ int s_wave[4];
  const int b = blockIdx.z, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int tx0 = blockIdx.x * kGraphTileW, ty0 = blockIdx.y * kGraphTileH;
  const int x = tx0 + (tid & 15) * 4, y = ty0 + (tid >> 4);
  for (int i = tid; i < kFontBytes; i += 256) s_font[i] = font[i];
  // offsets that do not describe the record array (a stale buffer) are cut to it: nothing is read outside `prims`
  const int lo = max(prim_off[b], 0), hi = min(prim_off[b + 1], n_prims);
  const bool mine = x < W && y < H;                  // W % 4 == 0: a lane's four pixels are inside together
  uint32_t rgb[4] = {background, background, background, background};
  int open = mine ? 4 : 0, decided = 0;              // bit j of `decided`: pixel x + j has its colour
  for (int end = hi; end > lo; end -= kGraphList) {
    const int i = end - 1 - tid;                     // thread 0 tests the pass's highest record
    int4 a = make_int4(0, 0, 0, 0), c = a, box = a;
    bool hit = false;
    if (i >= lo) {
      a = prims[2 * (int64_t)i];
      c = prims[2 * (int64_t)i + 1];
      const int kind = a.x & 15, t = (a.x >> 4) & 15;
      if (kind == kGraphSegment)
        box = make_int4(min(a.y, a.w) - t, min(a.z, c.x) - t, max(a.y, a.w) + t, max(a.z, c.x) + t);
      else if (kind == kGraphTriangle)
        box = make_int4(min(a.y, min(a.w, c.y)), min(a.z, min(c.x, c.z)), max(a.y, max(a.w, c.y)), max(a.z, max(c.x, c.z)));
      else
        box = make_int4(a.y, a.z, a.w, c.x);
      hit = box.x < tx0 + kGraphTileW && box.z >= tx0 && box.y < ty0 + kGraphTileH && box.w >= ty0;
    }
    const unsigned long long vote = __ballot(hit);
    if (lane == 0) s_wave[wave] = __popcll(vote);
    __syncthreads();
    int at = __popcll(vote & ((1ull << lane) - 1)), total = 0;
#pragma unroll
    for (int w = 0; w < 4; ++w) {
      const int n = s_wave[w];
      at += w < wave ? n : 0;
      total += n;
    }
    if (hit) {
      s_rec[2 * at] = a;
      s_rec[2 * at + 1] = c;
      s_box[at] = box;
    }
    __syncthreads();
    for (int k = 0; k < total && open; ++k) {        // the LDS reads are wave-uniform (one broadcast each)
      const int4 bx = s_box[k];
      if (y < bx.y || y > bx.w || x + 3 < bx.x || x > bx.z) continue;
      const int4 ra = s_rec[2 * k], rc = s_rec[2 * k + 1];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        if ((decided >> j) & 1) continue;
        bool ink;
        if (!graph_covers(ra, rc, x + j, y, text, text_bytes, s_font, ink)) continue;
        rgb[j] = ink ? (uint32_t)ra.x >> 8 : (uint32_t)rc.w;
        decided |= 1 << j;
        --open;
      }
    }
    // also the barrier between this pass's readers and the next pass's writers
    if (__syncthreads_count(open) == 0) break;
  }
  if (!mine) return;
  const int64_t npix = (int64_t)H * W;
  uint8_t* ob = out + (int64_t)b * 3 * npix + (int64_t)y * W + x;
#pragma unroll
  for (int ch = 0; ch < 3; ++ch) {
    uint32_t word = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) word |= ((rgb[j] >> (8 * ch)) & 0xffu) << (8 * j);
    *(uint32_t*)(ob + (int64_t)ch * npix) = word;
  }
}

}  // namespace csg

using namespace csg;

extern "C" {

int csg_draw_boxes_u8(const uint8_t* img, const float* boxes, const int64_t* objs, int64_t B, int64_t O, int64_t A, int64_t H,
                      int64_t W, int64_t image_id, const uint8_t* palette, int64_t P, int32_t thickness, uint8_t* out,
                      void* stream) {
  CSG_REQUIRE(B > 0 && B <= 65535 && H > 0 && W > 0 && W % 4 == 0 && H * W < (1ll << 31), CSG_E_BADSHAPE,
              "csg_draw_boxes_u8: bad shape B=%ld H=%ld W=%ld (W a multiple of 4)", (long)B, (long)H, (long)W);
  CSG_REQUIRE(O > 0 && A > 0 && P > 0 && thickness >= 1, CSG_E_BADSHAPE,
              "csg_draw_boxes_u8: bad shape O=%ld A=%ld P=%ld thickness=%d", (long)O, (long)A, (long)P, (int)thickness);
  CSG_REQUIRE(O <= kOverlayMaxRows && P <= kOverlayMaxColours, CSG_E_UNSUPPORTED,
              "csg_draw_boxes_u8: at most %d rows per sample and %d colours (got %ld, %ld)", kOverlayMaxRows,
              kOverlayMaxColours, (long)O, (long)P);
  CSG_REQUIRE(img != nullptr && boxes != nullptr && objs != nullptr && palette != nullptr && out != nullptr, CSG_E_BADSHAPE,
              "csg_draw_boxes_u8: null operand");
  CSG_REQUIRE(img != out, CSG_E_BADSHAPE, "csg_draw_boxes_u8: out must not be img");
  CSG_REQUIRE(((uintptr_t)img & 3) == 0 && ((uintptr_t)out & 3) == 0 && ((uintptr_t)boxes & 15) == 0, CSG_E_BADSHAPE,
              "csg_draw_boxes_u8: img and out must start on a 4-byte boundary, boxes on a 16-byte one");
  hipStream_t s = (hipStream_t)stream;
  const int64_t npix = H * W;
  ProfScope p(K_DRAW_BOXES, (double)B * npix * 6, s);
  int64_t blocks = cdiv(npix / 4, 256);
  if (blocks > 256) blocks = 256;
  CSG_LAUNCH(k_draw_boxes_u8, dim3((unsigned)blocks, (unsigned)B), dim3(256), 0, s, img, boxes, objs, (int)O, (int)A, (int)H,
             (int)W, image_id, palette, (int)P, (int)thickness, out);
  return check_launch("csg_draw_boxes_u8");
}

int csg_draw_labels_u8(const uint8_t* img, const float* boxes, const int64_t* objs, int64_t B, int64_t O, int64_t A, int64_t H,
                       int64_t W, int64_t image_id, const uint8_t* palette, int64_t P, const uint8_t* text,
                       const int32_t* text_off, const uint8_t* font, uint8_t* out, void* stream) {
  CSG_REQUIRE(B > 0 && B <= 65535 && H > 0 && W > 0 && W % 4 == 0 && H * W < (1ll << 31), CSG_E_BADSHAPE,
              "csg_draw_labels_u8: bad shape B=%ld H=%ld W=%ld (W a multiple of 4)", (long)B, (long)H, (long)W);
  CSG_REQUIRE(O > 0 && A > 0 && P > 0, CSG_E_BADSHAPE, "csg_draw_labels_u8: bad shape O=%ld A=%ld P=%ld", (long)O, (long)A,
              (long)P);
  CSG_REQUIRE(O <= kOverlayMaxRows && P <= kOverlayMaxColours, CSG_E_UNSUPPORTED,
              "csg_draw_labels_u8: at most %d rows per sample and %d colours (got %ld, %ld)", kOverlayMaxRows,
              kOverlayMaxColours, (long)O, (long)P);
  CSG_REQUIRE(img != nullptr && boxes != nullptr && objs != nullptr && palette != nullptr && text != nullptr &&
                  text_off != nullptr && font != nullptr && out != nullptr,
              CSG_E_BADSHAPE, "csg_draw_labels_u8: null operand");
  CSG_REQUIRE(img != out, CSG_E_BADSHAPE, "csg_draw_labels_u8: out must not be img");
  CSG_REQUIRE(((uintptr_t)img & 3) == 0 && ((uintptr_t)out & 3) == 0 && ((uintptr_t)boxes & 15) == 0 &&
                  ((uintptr_t)text_off & 3) == 0,
              CSG_E_BADSHAPE,
              "csg_draw_labels_u8: img, out and text_off must start on a 4-byte boundary, boxes on a 16-byte one");
  hipStream_t s = (hipStream_t)stream;
  const int64_t npix = H * W;
  ProfScope p(K_DRAW_LABELS, (double)B * npix * 6, s);
  int64_t blocks = cdiv(npix / 4, 256);
  if (blocks > 256) blocks = 256;
  CSG_LAUNCH(k_draw_labels_u8, dim3((unsigned)blocks, (unsigned)B), dim3(256), 0, s, img, boxes, objs, (int)O, (int)A, (int)H,
             (int)W, image_id, palette, (int)P, text, text_off, font, out);
  return check_launch("csg_draw_labels_u8");
}

int csg_draw_graph_u8(const int32_t* prims, int64_t n_prims, const int32_t* prim_off, const uint8_t* text,
                      int64_t text_bytes, const uint8_t* font, int64_t B, int64_t H, int64_t W, uint32_t background,
                      uint8_t* out, void* stream) {
  CSG_REQUIRE(B >= 1 && B <= 65535 && H >= 1 && H <= 2048 && W >= 1 && W <= 2048 && W % 4 == 0, CSG_E_BADSHAPE,
              "csg_draw_graph_u8: bad shape B=%ld H=%ld W=%ld (1 <= B <= 65535; H and W in [1, 2048], W a multiple of 4)",
              (long)B, (long)H, (long)W);
  CSG_REQUIRE(n_prims >= 0 && n_prims < (1ll << 30) && text_bytes >= 0, CSG_E_BADSHAPE,
              "csg_draw_graph_u8: bad sizes n_prims=%ld text_bytes=%ld", (long)n_prims, (long)text_bytes);
  CSG_REQUIRE(prims != nullptr && prim_off != nullptr && text != nullptr && font != nullptr && out != nullptr,
              CSG_E_BADSHAPE, "csg_draw_graph_u8: null operand");
  CSG_REQUIRE(((uintptr_t)prims & 15) == 0 && ((uintptr_t)prim_off & 3) == 0 && ((uintptr_t)out & 3) == 0, CSG_E_BADSHAPE,
              "csg_draw_graph_u8: prims must start on a 16-byte boundary, prim_off and out on a 4-byte one");
  hipStream_t s = (hipStream_t)stream;
  ProfScope p(K_DRAW_GRAPH, (double)B * H * W * 3, s);
  CSG_LAUNCH(k_draw_graph_u8, dim3((unsigned)cdiv(W, kGraphTileW), (unsigned)cdiv(H, kGraphTileH), (unsigned)B), dim3(256), 0,
             s, (const int4*)prims, (int)n_prims, prim_off, text, text_bytes, font, (int)H, (int)W, background, out);
  return check_launch("csg_draw_graph_u8");
}

}  // extern "C"
