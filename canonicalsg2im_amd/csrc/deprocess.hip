// Generated image -> uint8 picture: deprocess_batch(imgs, rescale, imagenet_deprocess) of the reference
// (sg2im/data/utils.py:36-65) on the device.  Per image and element, in exactly the reference's order (T.Normalize is
// sub_(mean).div_(std)):
//     t = x / inv_std[c]                (Normalize(mean 0, std INV_IMAGENET_STD);   x - 0 is x)
//     t = t - (-mean[c])                (Normalize(mean INV_IMAGENET_MEAN, std 1);  t / 1 is t)
//     t = (t - lo) / (hi - lo)          (rescale: lo, hi = min, max of the whole image after the two steps above)
//     u = byte(clamp(t * 255, 0, 255))  (truncation)
// Every step is one correctly rounded fp32 operation, as in torch on the host: this file is compiled with
// -ffp-contract=off (no multiply-add is formed) and hipcc's default correctly rounded fp32 division, so the bytes are
// those of the host code, not "close to" them.  min / max are exact whatever their association; they are formed as
// ordered trees (no atomics) and propagate NaN as torch.min / torch.max do.
#include "csg_common.h"

#include <math.h>

namespace csg {

struct DeprocConst {
  float div[3];   // INV_IMAGENET_STD as fp32
  float sub[3];   // INV_IMAGENET_MEAN as fp32
};

constexpr int kDeprocParts = 64;   // min / max partials per image: the apply pass folds them again (64 pairs per block)

__device__ __forceinline__ float min_nan(float a, float b) { return (a < b || a != a) ? a : b; }
__device__ __forceinline__ float max_nan(float a, float b) { return (a > b || a != a) ? a : b; }

__device__ __forceinline__ void wave_minmax(float& lo, float& hi) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    lo = min_nan(lo, __shfl_down(lo, off, 64));
    hi = max_nan(hi, __shfl_down(hi, off, 64));
  }
}

__device__ __forceinline__ void load_pixel(const float* __restrict__ p, int cs, float v[3]) {
  if (cs == 4) {
    const float4 q = *(const float4*)p;
    v[0] = q.x; v[1] = q.y; v[2] = q.z;
  } else {
    v[0] = p[0]; v[1] = p[1]; v[2] = p[2];
  }
}

// partial (B, kDeprocParts, 2) = [lo | hi] of a contiguous slice of image b's pixels after the two Normalize steps
__global__ __launch_bounds__(256) void k_deprocess_minmax(const float* __restrict__ img, int64_t npix, int cs, DeprocConst k,
                                                           float* __restrict__ partial) {
  __shared__ float s_lo[4], s_hi[4];
  const int b = blockIdx.y, part = blockIdx.x;
  const int64_t per = (npix + kDeprocParts - 1) / kDeprocParts;
  const int64_t p0 = (int64_t)part * per;
  const int64_t p1 = p0 + per < npix ? p0 + per : npix;
  const float* base = img + (int64_t)b * npix * cs;
  float lo = INFINITY, hi = -INFINITY;
  for (int64_t p = p0 + threadIdx.x; p < p1; p += 256) {
    float v[3];
    load_pixel(base + p * cs, cs, v);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      float t = v[c] / k.div[c];
      t = t - k.sub[c];
      lo = min_nan(lo, t);
      hi = max_nan(hi, t);
    }
  }
  wave_minmax(lo, hi);
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  if (lane == 0) { s_lo[w] = lo; s_hi[w] = hi; }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int q = 1; q < 4; ++q) { lo = min_nan(lo, s_lo[q]); hi = max_nan(hi, s_hi[q]); }
    float* o = partial + ((int64_t)b * kDeprocParts + part) * 2;
    o[0] = lo;
    o[1] = hi;
  }
}

// out (B,3,H,W) uint8 planar; a lane owns four consecutive pixels and writes one dword per plane
__global__ __launch_bounds__(256) void k_deprocess_apply(const float* __restrict__ img, int64_t npix, int cs, DeprocConst k,
                                                          const float* __restrict__ partial, uint8_t* __restrict__ out) {
  __shared__ float s_range[2];
  const int b = blockIdx.y;
  float lo = 0.f, span = 1.f;
  if (partial != nullptr) {
    if (threadIdx.x < 64) {
      float l = partial[((int64_t)b * kDeprocParts + threadIdx.x) * 2];
      float h = partial[((int64_t)b * kDeprocParts + threadIdx.x) * 2 + 1];
      wave_minmax(l, h);
      if (threadIdx.x == 0) { s_range[0] = l; s_range[1] = h - l; }
    }
    __syncthreads();
    lo = s_range[0];
    span = s_range[1];
  }
  const int64_t nquad = npix >> 2;
  const float* base = img + (int64_t)b * npix * cs;
  uint8_t* ob = out + (int64_t)b * 3 * npix;
  for (int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x; q < nquad; q += (int64_t)gridDim.x * 256) {
    uint32_t word[3] = {0u, 0u, 0u};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      float v[3];
      load_pixel(base + (q * 4 + j) * cs, cs, v);
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        float t = v[c] / k.div[c];
        t = t - k.sub[c];
        if (partial != nullptr) {
          t = t - lo;
          t = t / span;
        }
        t = t * 255.0f;
        // clamp(0, 255) keeps a NaN (torch.clamp does); byte() of a NaN is 0 on the x86 hosts torch runs on
        uint32_t u = 0u;
        if (t == t) {
          t = t < 0.f ? 0.f : t;
          t = t > 255.f ? 255.f : t;
          u = (uint32_t)t;
        }
        word[c] |= u << (8 * j);
      }
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) *(uint32_t*)(ob + (int64_t)c * npix + q * 4) = word[c];
  }
}

}  // namespace csg

using namespace csg;

extern "C" {

int64_t csg_deprocess_u8_workspace(int64_t B) { return B > 0 ? B * kDeprocParts * 2 * (int64_t)sizeof(float) : 0; }

int csg_deprocess_u8(const float* img, int64_t B, int64_t H, int64_t W, int64_t img_cs, const float* div3, const float* sub3,
                     int32_t rescale, uint8_t* out, float* workspace, int64_t workspace_bytes, void* stream) {
  CSG_REQUIRE(B > 0 && B <= 65535 && H > 0 && W > 0 && W % 4 == 0, CSG_E_BADSHAPE,
              "csg_deprocess_u8: bad shape B=%ld H=%ld W=%ld (W a multiple of 4)", (long)B, (long)H, (long)W);
  CSG_REQUIRE(img_cs == 3 || img_cs == 4, CSG_E_BADSHAPE, "csg_deprocess_u8: img_cs = %ld, 3 or 4 floats per pixel",
              (long)img_cs);
  CSG_REQUIRE(img != nullptr && out != nullptr && div3 != nullptr && sub3 != nullptr, CSG_E_BADSHAPE,
              "csg_deprocess_u8: null operand");
  CSG_REQUIRE(!rescale || (workspace != nullptr && workspace_bytes >= csg_deprocess_u8_workspace(B)), CSG_E_WORKSPACE,
              "csg_deprocess_u8: rescale needs csg_deprocess_u8_workspace(B) bytes");
  DeprocConst k;
  for (int c = 0; c < 3; ++c) {
    k.div[c] = div3[c];
    k.sub[c] = sub3[c];
  }
  hipStream_t s = (hipStream_t)stream;
  const int64_t npix = H * W;
  ProfScope p(K_DEPROCESS, (double)B * npix * (img_cs * 4 * (rescale ? 2 : 1) + 3), s);
  if (rescale)
    CSG_LAUNCH(k_deprocess_minmax, dim3(kDeprocParts, (unsigned)B), dim3(256), 0, s, img, npix, (int)img_cs, k, workspace);
  int64_t blocks = cdiv(npix / 4, 256);
  if (blocks > 256) blocks = 256;
  CSG_LAUNCH(k_deprocess_apply, dim3((unsigned)blocks, (unsigned)B), dim3(256), 0, s, img, npix, (int)img_cs, k,
             rescale ? (const float*)workspace : (const float*)nullptr, out);
  return check_launch("csg_deprocess_u8");
}

}  // extern "C"
