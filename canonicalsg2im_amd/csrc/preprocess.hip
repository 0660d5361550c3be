// Decoded pictures -> the trainer's image tensor: the per-sample transform of the reference's loader
// (sg2im/data/packed_coco.py:269-272, T.Resize + T.ToTensor + T.Normalize) for a batch of differently sized images.
//
// T.Resize on a PIL image is Pillow's 8-bit `resize((W, H), BILINEAR)`.  Per axis (inS -> outS), in fp64:
//     scale = inS / outS;  fs = max(scale, 1);  support = fs;  ss = 1 / fs
//     output xx:  c = (xx + 0.5) * scale;  xmin = max(int(c - support + 0.5), 0);  xmax = min(int(c + support + 0.5), inS)
//                 w_x = 1 - |(x + xmin - c + 0.5) * ss|  where that magnitude is below 1, else 0     (x = 0 .. xmax - xmin - 1)
//                 ww = the w_x summed in tap order;  w_x / ww;  coefficient = int(0.5 + w * 2^22)  (truncation)
//     pass:       byte = clip((2^21 + sum pixel * coefficient) >> 22, 0, 255)                        (integers)
// The horizontal pass runs first and leaves a uint8 image; the vertical pass reads that image.  A pass whose size does
// not change is skipped (NOT run with identity coefficients).  The fp64 operations are add, multiply, divide, compare
// and truncation: with -ffp-contract=off (this file's flag in the build) each is the correctly rounded operation the
// host performs, so the coefficients — computed here, by the block that uses them, into LDS — are the host's integers
// and the bytes are Pillow's bytes.
// ToTensor + Normalize are three fp32 operations per element: float(byte) / 255, - mean[c], / std[c]: torch's bits.
//
// Two entry points share every kernel below as the two instantiations of one template.  csg_preprocess (kPx = false):
// descriptor rows (offset, h, w), 3-byte pixels as a compile-time constant: signature and bits unchanged.  csg_preprocess_px (kPx =
// true): rows (offset, h, w, bytes per pixel), 3 or 4 per picture.  A 4-byte pixel is R, G, B and a byte that is ignored
// (what Pillow's RGBA -> RGB conversion drops); the pass that reads the picture itself loads such a pixel as one dword
// when the picture starts on a dword boundary, byte by byte otherwise.  The horizontal result is 3 bytes per pixel always.
#include "csg_common.h"

namespace csg {

constexpr int kPreMaxScale = CSG_PREPROCESS_MAX_SCALE;   // fs <= 64
constexpr int kPreMaxTaps = 2 * kPreMaxScale + 1;         // Pillow's ksize = 2 * ceil(support) + 1
constexpr int kPreMaxSide = CSG_PREPROCESS_MAX_SIDE;
constexpr int kPrecisionBits = 22;                        // 32 - 8 - 2
constexpr int kHCols = 64;                                // horizontal pass: output columns per block (one LDS column each)
constexpr int kHRows = 16;                                //                  source rows per block
constexpr int kVRows = 8;                                 // vertical pass: output rows per block

struct PreConst {
  float sub[3];
  float div[3];
};

struct PreImage {
  int64_t off;      // first byte of the picture in src
  int64_t ws_off;   // first byte of its horizontal result in the workspace
  int h, w;
  int bpp;          // bytes per pixel of the picture in src: 3, or 4 (kPx only)
  bool ok;
};

// The descriptor row of image b and the workspace offset that follows from the rows before it.  The host validated the
// HOST copy of the descriptor; a device row that disagrees with it (a stale buffer under a replayed graph) must still
// not read or write out of bounds: such an image is skipped.  The walk over the rows before b is one lane's work
// (block_image): B rows of three loads, not B rows per thread.
template <bool kPx>
__device__ __forceinline__ PreImage load_image(const int64_t* __restrict__ desc, int b, int H, int W, int64_t src_bytes,
                                               int64_t ws_bytes, int max_h) {
  constexpr int kRow = kPx ? 4 : 3;                    // int64 entries per descriptor row
  PreImage im;
  int64_t ws = 0;
  bool ok = true;
  for (int j = 0; j <= b; ++j) {
    const int64_t off = desc[kRow * j], h = desc[kRow * j + 1], w = desc[kRow * j + 2];
    const int64_t bpp = kPx ? desc[kRow * j + 3] : 3;
    const bool good = h >= 1 && h <= kPreMaxSide && w >= 1 && w <= kPreMaxSide && h <= (int64_t)kPreMaxScale * H &&
                      w <= (int64_t)kPreMaxScale * W && (bpp == 3 || bpp == 4) && off >= 0 && off + bpp * h * w <= src_bytes;
    if (j == b) {
      im.off = off;
      im.h = (int)h;
      im.w = (int)w;
      im.bpp = (int)bpp;
      im.ws_off = ws;
      ok = ok && good && h <= max_h && (w == W || ws + 3 * h * W <= ws_bytes);
    } else {
      ok = ok && good;                       // a bad row before this one makes this one's workspace offset meaningless
      ws += good ? 3 * h * W : 0;
    }
  }
  im.ok = ok;
  return im;
}

// load_image by lane 0, handed to the block through LDS (one barrier)
template <bool kPx>
__device__ __forceinline__ PreImage block_image(PreImage* s_im, const int64_t* __restrict__ desc, int b, int H, int W,
                                                int64_t src_bytes, int64_t ws_bytes, int max_h) {
  if (threadIdx.x == 0) *s_im = load_image<kPx>(desc, b, H, W, src_bytes, ws_bytes, max_h);
  __syncthreads();
  return *s_im;
}

// Coefficients of output index xx of an axis inS -> outS into k[0 .. n) (stride `ks` ints); returns the first tap, n by
// reference.  One lane, serial: ww is a sum in tap order.
__device__ __forceinline__ int axis_coefficients(int inS, int outS, int xx, int* __restrict__ k, int ks, int& n) {
  const double scale = (double)inS / (double)outS;
  const double fs = scale < 1.0 ? 1.0 : scale;
  const double support = fs;
  const double ss = 1.0 / fs;
  const double c = ((double)xx + 0.5) * scale;
  int xmin = (int)(c - support + 0.5);
  if (xmin < 0) xmin = 0;
  int xmax = (int)(c + support + 0.5);
  if (xmax > inS) xmax = inS;
  int cnt = xmax - xmin;
  if (cnt > kPreMaxTaps) cnt = kPreMaxTaps;              // cannot happen for fs <= kPreMaxScale; keeps the LDS column
  if (cnt < 0) cnt = 0;
  double ww = 0.0;
  for (int x = 0; x < cnt; ++x) {
    double a = ((double)(x + xmin) - c + 0.5) * ss;
    if (a < 0.0) a = -a;
    ww += a < 1.0 ? 1.0 - a : 0.0;
  }
  for (int x = 0; x < cnt; ++x) {
    double a = ((double)(x + xmin) - c + 0.5) * ss;
    if (a < 0.0) a = -a;
    double w = a < 1.0 ? 1.0 - a : 0.0;
    if (ww != 0.0) w = w / ww;
    k[x * ks] = w < 0.0 ? (int)(-0.5 + w * (double)(1 << kPrecisionBits)) : (int)(0.5 + w * (double)(1 << kPrecisionBits));
  }
  n = cnt;
  return xmin;
}

__device__ __forceinline__ uint32_t clip8(int acc) {
  const int v = acc >> kPrecisionBits;
  return (uint32_t)(v < 0 ? 0 : (v > 255 ? 255 : v));
}

// R | G << 8 | B << 16 of the 4-byte pixel at p: one dword load when the picture is dword-aligned (then every pixel is)
__device__ __forceinline__ uint32_t load_px4(const uint8_t* __restrict__ p, bool dword) {
  if (dword) return *(const uint32_t*)p & 0xffffffu;
  return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16);
}

// the first npx of four consecutive pixels at p as twelve channel values (zeros beyond)
template <bool kPx>
__device__ __forceinline__ void load_quad(const uint8_t* __restrict__ p, int npx, int bpp, bool dword, uint32_t (&v)[12]) {
  if (kPx && bpp == 4) {
#pragma unroll
    for (int px = 0; px < 4; ++px) {
      const uint32_t word = px < npx ? load_px4(p + 4 * px, dword) : 0u;
      v[3 * px] = word & 255u;
      v[3 * px + 1] = (word >> 8) & 255u;
      v[3 * px + 2] = word >> 16;
    }
  } else {
#pragma unroll
    for (int e = 0; e < 12; ++e) v[e] = e < npx * 3 ? (uint32_t)p[e] : 0u;
  }
}

// ws (h_b, W, 3) uint8 of every image with w_b != W.  Block = (64 output columns, 16 source rows, image); a lane owns
// four consecutive bytes of a row's 192-byte strip and stores them as one dword when the rows are dword-aligned (W % 4 == 0).
template <bool kPx>
__global__ __launch_bounds__(256) void k_preprocess_horizontal(const uint8_t* __restrict__ src, const int64_t* __restrict__ desc,
                                                                int H, int W, int64_t src_bytes, int64_t ws_bytes, int max_h,
                                                                uint8_t* __restrict__ ws) {
  __shared__ int s_coef[kPreMaxTaps * kHCols];            // tap-major: lanes of neighbouring columns, neighbouring banks
  __shared__ int s_min[kHCols], s_cnt[kHCols];
  __shared__ PreImage s_im;
  const int b = blockIdx.z;
  const PreImage im = block_image<kPx>(&s_im, desc, b, H, W, src_bytes, ws_bytes, max_h);
  const int y0 = blockIdx.y * kHRows, x0 = blockIdx.x * kHCols;
  if (!im.ok || im.w == W || y0 >= im.h) return;          // block-uniform
  const int cols = W - x0 < kHCols ? W - x0 : kHCols;
  if ((int)threadIdx.x < cols) {
    int n;
    s_min[threadIdx.x] = axis_coefficients(im.w, W, x0 + threadIdx.x, s_coef + threadIdx.x, kHCols, n);
    s_cnt[threadIdx.x] = n;
  }
  __syncthreads();
  const int rows = im.h - y0 < kHRows ? im.h - y0 : kHRows;
  const bool wide = (W & 3) == 0;                         // then cols * 3 is a multiple of 4 and every row starts on a dword
  const int quads = (cols * 3 + 3) >> 2;
  const uint8_t* in = src + im.off;
  uint8_t* out = ws + im.ws_off;
  if (kPx && im.bpp == 4) {                               // block-uniform
    // the lane's four bytes lie in at most two output columns: one walk over a column's taps serves its three channels
    const bool dword = (im.off & 3) == 0;
    for (int q = threadIdx.x; q < rows * quads; q += 256) {
      const int r = q / quads, d = q - r * quads;
      const uint8_t* row = in + (int64_t)(y0 + r) * im.w * 4;
      uint8_t* orow = out + ((int64_t)(y0 + r) * W + x0) * 3;
      uint32_t word = 0u;
      int have = -1;
      uint32_t rgb = 0u;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int e = d * 4 + j;
        if (e < cols * 3) {
          const int col = e / 3, ch = e - col * 3;
          if (col != have) {
            const int n = s_cnt[col];
            const uint8_t* p = row + (int64_t)s_min[col] * 4;
            int a0 = 1 << (kPrecisionBits - 1), a1 = a0, a2 = a0;
            for (int k = 0; k < n; ++k) {
              const uint32_t px = load_px4(p + 4 * k, dword);
              const int c = s_coef[k * kHCols + col];
              a0 += (int)(px & 255u) * c;
              a1 += (int)((px >> 8) & 255u) * c;
              a2 += (int)(px >> 16) * c;
            }
            rgb = clip8(a0) | (clip8(a1) << 8) | (clip8(a2) << 16);
            have = col;
          }
          const uint32_t u = (rgb >> (8 * ch)) & 255u;
          if (wide) word |= u << (8 * j);
          else orow[e] = (uint8_t)u;
        }
      }
      if (wide) *(uint32_t*)(orow + d * 4) = word;
    }
    return;
  }
  for (int q = threadIdx.x; q < rows * quads; q += 256) {
    const int r = q / quads, d = q - r * quads;
    const uint8_t* row = in + (int64_t)(y0 + r) * im.w * 3;
    uint8_t* orow = out + ((int64_t)(y0 + r) * W + x0) * 3;
    uint32_t word = 0u;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int e = d * 4 + j;
      if (e < cols * 3) {
        const int col = e / 3, ch = e - col * 3;
        const int n = s_cnt[col];
        const uint8_t* p = row + s_min[col] * 3 + ch;
        int acc = 1 << (kPrecisionBits - 1);
        for (int k = 0; k < n; ++k) acc += (int)p[k * 3] * s_coef[k * kHCols + col];
        const uint32_t u = clip8(acc);
        if (wide) word |= u << (8 * j);
        else orow[e] = (uint8_t)u;
      }
    }
    if (wide) *(uint32_t*)(orow + d * 4) = word;
  }
}

// out (B,3,H,W) fp32 planar and, when given, out_u8 (B,H,W,3).  Block = (8 output rows, image); a lane owns four consecutive
// pixels of a row: twelve bytes from each tap's row, three float4 stores (one per plane) and three dwords of out_u8 when
// W % 4 == 0, single elements otherwise.  Reads the horizontal result, or the picture itself when w_b == W.
template <bool kPx>
__global__ __launch_bounds__(256) void k_preprocess_vertical(const uint8_t* __restrict__ src, const int64_t* __restrict__ desc,
                                                              int H, int W, int64_t src_bytes, int64_t ws_bytes, int max_h,
                                                              const uint8_t* __restrict__ ws, PreConst kc,
                                                              float* __restrict__ out, uint8_t* __restrict__ out_u8) {
  __shared__ int s_coef[kVRows * kPreMaxTaps];
  __shared__ int s_min[kVRows], s_cnt[kVRows];
  __shared__ PreImage s_im;
  const int b = blockIdx.y;
  const PreImage im = block_image<kPx>(&s_im, desc, b, H, W, src_bytes, ws_bytes, max_h);
  if (!im.ok) return;                                     // block-uniform
  const int y0 = blockIdx.x * kVRows;
  const int rows = H - y0 < kVRows ? H - y0 : kVRows;
  const bool resample = im.h != H;
  if (resample && (int)threadIdx.x < rows) {
    int n;
    s_min[threadIdx.x] = axis_coefficients(im.h, H, y0 + threadIdx.x, s_coef + threadIdx.x * kPreMaxTaps, 1, n);
    s_cnt[threadIdx.x] = n;
  }
  __syncthreads();
  const uint8_t* in = im.w == W ? src + im.off : ws + im.ws_off;
  const int bpp = (kPx && im.w == W) ? im.bpp : 3;        // of what this pass reads: the horizontal result has 3
  const bool dword = kPx && (im.off & 3) == 0;            // only looked at for 4-byte pixels, i.e. when reading src
  const int64_t rowb = (int64_t)W * bpp;
  const bool wide = (W & 3) == 0;
  const int quads = (W + 3) >> 2;
  const int64_t plane = (int64_t)H * W;
  float* ob = out + (int64_t)b * 3 * plane;
  uint8_t* ub = out_u8 != nullptr ? out_u8 + (int64_t)b * plane * 3 : nullptr;
  for (int q = threadIdx.x; q < rows * quads; q += 256) {
    const int r = q / quads, x = (q - r * quads) * 4;
    const int yy = y0 + r;
    const int npx = W - x < 4 ? W - x : 4;
    uint32_t u[12];
    if (resample) {
      const int n = s_cnt[r];
      const int* kk = s_coef + r * kPreMaxTaps;
      const uint8_t* p = in + (int64_t)s_min[r] * rowb + x * bpp;
      int acc[12];
#pragma unroll
      for (int e = 0; e < 12; ++e) acc[e] = 1 << (kPrecisionBits - 1);
      for (int k = 0; k < n; ++k) {
        const int c = kk[k];
        uint32_t v[12];
        load_quad<kPx>(p, npx, bpp, dword, v);
#pragma unroll
        for (int e = 0; e < 12; ++e) acc[e] += (int)v[e] * c;
        p += rowb;
      }
#pragma unroll
      for (int e = 0; e < 12; ++e) u[e] = clip8(acc[e]);
    } else {
      load_quad<kPx>(in + (int64_t)yy * rowb + x * bpp, npx, bpp, dword, u);
    }
    float f[12];
#pragma unroll
    for (int e = 0; e < 12; ++e) {
      const int ch = e % 3;
      float t = (float)u[e] / 255.0f;                     // ToTensor
      t = t - kc.sub[ch];                                 // Normalize: sub_(mean)
      f[e] = t / kc.div[ch];                              //            div_(std)
    }
    const int64_t o = (int64_t)yy * W + x;
    if (wide) {
#pragma unroll
      for (int ch = 0; ch < 3; ++ch)
        *(float4*)(ob + ch * plane + o) = make_float4(f[ch], f[3 + ch], f[6 + ch], f[9 + ch]);
      if (ub != nullptr) {
#pragma unroll
        for (int d = 0; d < 3; ++d)
          *(uint32_t*)(ub + o * 3 + d * 4) = u[4 * d] | (u[4 * d + 1] << 8) | (u[4 * d + 2] << 16) | (u[4 * d + 3] << 24);
      }
    } else {
#pragma unroll
      for (int e = 0; e < 12; ++e) {
        if (e < npx * 3) {
          ob[(e % 3) * plane + o + e / 3] = f[e];
          if (ub != nullptr) ub[o * 3 + e] = (uint8_t)u[e];
        }
      }
    }
  }
}

// host: the descriptor's rows (`row` int64 entries each: 3, or 4 with the bytes per pixel) are inside the stated range and
// inside src
static int check_desc(const char* who, const int64_t* desc, int row, int64_t B, int64_t H, int64_t W, int64_t src_bytes,
                      int64_t* max_h, int64_t* ws) {
  CSG_REQUIRE(desc != nullptr, CSG_E_BADSHAPE, "%s: null host descriptor", who);
  CSG_REQUIRE(B >= 1 && B <= CSG_PREPROCESS_MAX_BATCH, CSG_E_BADSHAPE, "%s: B = %ld, 1 .. %d images per call", who, (long)B,
              CSG_PREPROCESS_MAX_BATCH);
  CSG_REQUIRE(H >= 1 && H <= kPreMaxSide && W >= 1 && W <= kPreMaxSide, CSG_E_BADSHAPE, "%s: output %ld x %ld, sides 1 .. %d",
              who, (long)H, (long)W, kPreMaxSide);
  *max_h = 0;
  *ws = 0;
  for (int64_t i = 0; i < B; ++i) {
    const int64_t off = desc[row * i], h = desc[row * i + 1], w = desc[row * i + 2];
    const int64_t bpp = row == 4 ? desc[row * i + 3] : 3;
    CSG_REQUIRE(h >= 1 && h <= kPreMaxSide && w >= 1 && w <= kPreMaxSide, CSG_E_BADSHAPE,
                "%s: image %ld is %ld x %ld, sides 1 .. %d", who, (long)i, (long)h, (long)w, kPreMaxSide);
    CSG_REQUIRE(bpp == 3 || bpp == 4, CSG_E_BADSHAPE, "%s: image %ld has %ld bytes per pixel, 3 or 4", who, (long)i, (long)bpp);
    CSG_REQUIRE(h <= kPreMaxScale * H && w <= kPreMaxScale * W, CSG_E_UNSUPPORTED,
                "%s: image %ld (%ld x %ld -> %ld x %ld) shrinks an axis by more than %d", who, (long)i, (long)h, (long)w, (long)H,
                (long)W, kPreMaxScale);
    CSG_REQUIRE(off >= 0 && off + bpp * h * w <= src_bytes, CSG_E_BADSHAPE,
                "%s: image %ld (offset %ld, %ld x %ld x %ld bytes) leaves the %ld source bytes", who, (long)i, (long)off, (long)h,
                (long)w, (long)bpp, (long)src_bytes);
    if (h > *max_h) *max_h = h;
    *ws += 3 * h * W;
  }
  return CSG_OK;
}

template <bool kPx>
static int preprocess(const char* who, const uint8_t* src, int64_t src_bytes, const int64_t* desc, const int64_t* desc_host,
                      int64_t B, int64_t H, int64_t W, const float* sub3, const float* div3, float* out, uint8_t* out_u8,
                      uint8_t* workspace, int64_t workspace_bytes, void* stream) {
  int64_t max_h = 0, need = 0;
  const int rc = check_desc(who, desc_host, kPx ? 4 : 3, B, H, W, src_bytes, &max_h, &need);
  if (rc != CSG_OK) return rc;
  CSG_REQUIRE(src != nullptr && desc != nullptr && out != nullptr && sub3 != nullptr && div3 != nullptr, CSG_E_BADSHAPE,
              "%s: null operand", who);
  CSG_REQUIRE(((uintptr_t)out & 15) == 0 && ((uintptr_t)out_u8 & 3) == 0 && ((uintptr_t)workspace & 3) == 0, CSG_E_BADSHAPE,
              "%s: out must be 16-byte aligned, out_u8 and workspace 4-byte aligned (float4 / dword stores)", who);
  CSG_REQUIRE(!kPx || ((uintptr_t)src & 3) == 0, CSG_E_BADSHAPE,
              "%s: src must be 4-byte aligned (dword loads of 4-byte pixels at offsets that are multiples of 4)", who);
  CSG_REQUIRE(workspace != nullptr && workspace_bytes >= need, CSG_E_WORKSPACE,
              "%s: %s_workspace(...) = %ld bytes are needed, %ld given", who, who, (long)need, (long)workspace_bytes);
  PreConst kc;
  for (int c = 0; c < 3; ++c) {
    kc.sub[c] = sub3[c];
    kc.div[c] = div3[c];
  }
  hipStream_t s = (hipStream_t)stream;
  ProfScope p(K_PREPROCESS, (double)src_bytes + 2.0 * (double)need + (double)B * H * W * 3 * (4 + (out_u8 ? 1 : 0)), s);
  // always both launches, whatever the widths of THIS batch: a captured pair must serve a later batch whose w_i != W
  CSG_LAUNCH(k_preprocess_horizontal<kPx>, dim3((unsigned)cdiv(W, kHCols), (unsigned)cdiv(max_h, kHRows), (unsigned)B),
             dim3(256), 0, s, src, desc, (int)H, (int)W, src_bytes, workspace_bytes, (int)max_h, workspace);
  CSG_LAUNCH(k_preprocess_vertical<kPx>, dim3((unsigned)cdiv(H, kVRows), (unsigned)B), dim3(256), 0, s, src, desc, (int)H, (int)W,
             src_bytes, workspace_bytes, (int)max_h, (const uint8_t*)workspace, kc, out, out_u8);
  return check_launch(who);
}

static int64_t workspace_bytes_of(const int64_t* desc_host, int row, int64_t B, int64_t W) {
  if (desc_host == nullptr || B < 1 || W < 1) return 0;
  int64_t n = 0;
  for (int64_t i = 0; i < B; ++i) n += desc_host[row * i + 1] > 0 ? 3 * desc_host[row * i + 1] * W : 0;
  return n;
}

}  // namespace csg

using namespace csg;

extern "C" {

int64_t csg_preprocess_workspace(const int64_t* desc_host, int64_t B, int64_t W) { return workspace_bytes_of(desc_host, 3, B, W); }

int csg_preprocess(const uint8_t* src, int64_t src_bytes, const int64_t* desc, const int64_t* desc_host, int64_t B, int64_t H,
                   int64_t W, const float* sub3, const float* div3, float* out, uint8_t* out_u8, uint8_t* workspace,
                   int64_t workspace_bytes, void* stream) {
  return preprocess<false>("csg_preprocess", src, src_bytes, desc, desc_host, B, H, W, sub3, div3, out, out_u8, workspace,
                           workspace_bytes, stream);
}

int64_t csg_preprocess_px_workspace(const int64_t* desc_host, int64_t B, int64_t W) {
  return workspace_bytes_of(desc_host, 4, B, W);
}

int csg_preprocess_px(const uint8_t* src, int64_t src_bytes, const int64_t* desc, const int64_t* desc_host, int64_t B, int64_t H,
                      int64_t W, const float* sub3, const float* div3, float* out, uint8_t* out_u8, uint8_t* workspace,
                      int64_t workspace_bytes, void* stream) {
  return preprocess<true>("csg_preprocess_px", src, src_bytes, desc, desc_host, B, H, W, sub3, div3, out, out_u8, workspace,
                          workspace_bytes, stream);
}

}  // extern "C"
