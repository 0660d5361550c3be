// Exponential moving average of the model's weights: update, swap and fill of a flat fp32 shadow, ONE launch per call
// whatever the number of tensors (include/csg_hip.h, "EMA of the weights").
//
// THE TABLE LIVES IN DEVICE MEMORY.  The other multi-tensor entries of this library (csg_wino_pack_weights_multi,
// csg_spectral_norm_fwd_multi, csg_hinge_mean_fwd) carry their items in the kernel's arguments, 24-32 per launch: their item
// lists change from call to call.  This one is built once, when the shadow is made — a model has a few hundred tensors and
// their storage stays where it is — so the items are uploaded once and every later call is one launch that reads them
// from memory, not one launch per 32 items.
//
// Work split.  An item of numel floats is cut into ceil(numel / CSG_EMA_CHUNK) chunks of CSG_EMA_CHUNK = 4096 floats (16 KB
// per stream); a chunk never spans two items, an empty item has none.  chunk0 of an item is the number of chunks before it.
// A block of 256 lanes owns a chunk at a time: it finds the chunk's item by bisection over chunk0 (the chunk index is
// uniform over the block: scalar loads), then every lane moves 16 bytes per stream and iteration, four iterations with all
// loads issued before the first store — 8 x 16 bytes in flight per lane on the averaging path.  The grid is min(chunks, 2048)
// blocks, eight per CU on 256 CUs, and strides over the rest.  The last numel % 4 floats of an item go one per lane.
//
// Arithmetic (kind AVERAGE, mode UPDATE), the contract the tests' bound is derived from:
//     t  = omd * p          one fp32 multiplication, rounded
//     e' = fmaf(d, e, t)    one fused multiply-add, rounded once
// d and omd are host-made scalars.  omd == 0 (a decay of exactly 1) touches no AVERAGE item at all: e + 0 * p would turn
// -0 into +0 and any e into NaN beside an infinite p.  Everything else — kind COPY, SWAP, FILL — moves bits and computes
// nothing: NaN payloads and signed zeros arrive as they left.  No atomics, no host synchronisation, nothing read back.
// Compiled with -ffp-contract=off: the two operations above stay two.
#include "csg_common.h"
#include "csg_vec4.h"

namespace csg {

constexpr int kEmaThreads = 256;
constexpr int kEmaIters = CSG_EMA_CHUNK / (4 * kEmaThreads);
constexpr int kEmaMaxGrid = 2048;
static_assert(kEmaIters * 4 * kEmaThreads == CSG_EMA_CHUNK, "a chunk is a whole number of 16-byte sweeps of the block");

template <int MODE>
__device__ __forceinline__ float ema_one(float p, float e, bool average, float d, float omd) {
  if (MODE == CSG_EMA_UPDATE && average) return __fmaf_rn(d, e, __fmul_rn(omd, p));
  return p;
}

template <int MODE>
__global__ __launch_bounds__(kEmaThreads) void k_ema(const csg_ema_item* __restrict__ items, int n, long long chunks, float d,
                                                     float omd) {
  const int tid = threadIdx.x;
  for (long long c = blockIdx.x; c < chunks; c += gridDim.x) {
    // the last item whose chunk0 <= c: empty items share their successor's chunk0 and are stepped over
    int lo = 0, hi = n;
    while (hi - lo > 1) {
      const int mid = (lo + hi) >> 1;
      if (items[mid].chunk0 <= c) lo = mid; else hi = mid;
    }
    const csg_ema_item it = items[lo];
    const long long off = (c - it.chunk0) * (long long)CSG_EMA_CHUNK;
    long long rem = it.numel - off;
    if (rem <= 0) continue;                           // (a table that disagrees with its own chunk0: touch nothing)
    if (rem > CSG_EMA_CHUNK) rem = CSG_EMA_CHUNK;
    const bool average = it.kind == CSG_EMA_AVERAGE;
    if (MODE == CSG_EMA_UPDATE && average && omd == 0.0f) continue;
    float* __restrict__ p = it.src + off;
    float* __restrict__ e = it.dst + off;
    const int nv = (int)(rem >> 2);
    const bool need_e = MODE == CSG_EMA_SWAP || (MODE == CSG_EMA_UPDATE && average);
    float4 pv[kEmaIters], ev[kEmaIters];
#pragma unroll
    for (int k = 0; k < kEmaIters; ++k) {
      const int i = tid + k * kEmaThreads;
      if (i < nv) {
        pv[k] = ld4(p + 4 * i);
        ev[k] = need_e ? ld4(e + 4 * i) : pv[k];
      }
    }
#pragma unroll
    for (int k = 0; k < kEmaIters; ++k) {
      const int i = tid + k * kEmaThreads;
      if (i < nv) {
        float4 o;
        o.x = ema_one<MODE>(pv[k].x, ev[k].x, average, d, omd);
        o.y = ema_one<MODE>(pv[k].y, ev[k].y, average, d, omd);
        o.z = ema_one<MODE>(pv[k].z, ev[k].z, average, d, omd);
        o.w = ema_one<MODE>(pv[k].w, ev[k].w, average, d, omd);
        st4(e + 4 * i, o);
        if (MODE == CSG_EMA_SWAP) st4(p + 4 * i, ev[k]);
      }
    }
    const int j = 4 * nv + tid;                       // the item's tail: at most three floats, in its last chunk
    if (tid < (int)(rem & 3)) {
      const float ps = p[j];
      const float es = need_e ? e[j] : 0.0f;
      e[j] = ema_one<MODE>(ps, es, average, d, omd);
      if (MODE == CSG_EMA_SWAP) p[j] = es;
    }
  }
}

}  // namespace csg

using namespace csg;

extern "C" {

int64_t csg_ema_table_plan(csg_ema_item* items, int64_t n) {
  CSG_REQUIRE(items != nullptr && n >= 1 && n <= CSG_EMA_MAX_ITEMS, CSG_E_BADSHAPE,
              "csg_ema_table_plan: %ld items (1 .. %d)", (long)n, CSG_EMA_MAX_ITEMS);
  int64_t chunks = 0;
  for (int64_t i = 0; i < n; ++i) {
    csg_ema_item& it = items[i];
    CSG_REQUIRE(it.numel >= 0 && it.numel <= ((int64_t)1 << 40), CSG_E_BADSHAPE, "csg_ema_table_plan: item %ld has %ld elements",
                (long)i, (long)it.numel);
    CSG_REQUIRE(it.kind == CSG_EMA_AVERAGE || it.kind == CSG_EMA_COPY, CSG_E_BADSHAPE,
                "csg_ema_table_plan: item %ld has kind %d (0 = average, 1 = copy)", (long)i, (int)it.kind);
    CSG_REQUIRE(it.numel == 0 || (it.src != nullptr && it.dst != nullptr), CSG_E_BADSHAPE,
                "csg_ema_table_plan: item %ld has a null pointer", (long)i);
    CSG_REQUIRE(it.numel == 0 || (((uintptr_t)it.src | (uintptr_t)it.dst) & 15) == 0, CSG_E_BADSHAPE,
                "csg_ema_table_plan: item %ld: source and shadow slot must be 16-byte aligned", (long)i);
    it.chunk0 = chunks;
    it.reserved = 0;
    chunks += cdiv(it.numel, (int64_t)CSG_EMA_CHUNK);
  }
  return chunks;
}

int csg_ema_apply(const csg_ema_item* items, int64_t n, int64_t chunks, int32_t mode, float d, float omd, void* stream) {
  CSG_REQUIRE(mode == CSG_EMA_UPDATE || mode == CSG_EMA_SWAP || mode == CSG_EMA_FILL, CSG_E_BADSHAPE,
              "csg_ema_apply: mode %d (0 = update, 1 = swap, 2 = fill)", (int)mode);
  CSG_REQUIRE(items != nullptr && n >= 1 && n <= CSG_EMA_MAX_ITEMS && chunks >= 0, CSG_E_BADSHAPE,
              "csg_ema_apply: %ld items (1 .. %d), %ld chunks", (long)n, CSG_EMA_MAX_ITEMS, (long)chunks);
  CSG_REQUIRE(((uintptr_t)items & 7) == 0, CSG_E_BADSHAPE, "csg_ema_apply: the table must be 8-byte aligned");
  if (mode == CSG_EMA_UPDATE)                         // (!(x) so that a NaN is refused too)
    CSG_REQUIRE(d >= 0.0f && d <= 1.0f && omd >= 0.0f && omd <= 1.0f, CSG_E_BADSHAPE,
                "csg_ema_apply: d = %g and omd = %g must lie in [0, 1]", (double)d, (double)omd);
  if (chunks == 0) return CSG_OK;                     // every item is empty
  hipStream_t s = (hipStream_t)stream;
  const unsigned grid = (unsigned)(chunks < kEmaMaxGrid ? chunks : kEmaMaxGrid);
  ProfScope p(K_EMA, (double)chunks * CSG_EMA_CHUNK * (mode == CSG_EMA_FILL ? 8.0 : mode == CSG_EMA_SWAP ? 16.0 : 12.0), s);
  if (mode == CSG_EMA_UPDATE)
    CSG_LAUNCH(k_ema<CSG_EMA_UPDATE>, dim3(grid), dim3(kEmaThreads), 0, s, items, (int)n, (long long)chunks, d, omd);
  else if (mode == CSG_EMA_SWAP)
    CSG_LAUNCH(k_ema<CSG_EMA_SWAP>, dim3(grid), dim3(kEmaThreads), 0, s, items, (int)n, (long long)chunks, d, omd);
  else
    CSG_LAUNCH(k_ema<CSG_EMA_FILL>, dim3(grid), dim3(kEmaThreads), 0, s, items, (int)n, (long long)chunks, d, omd);
  return check_launch("csg_ema_apply");
}

}  // extern "C"
