// Graph rewriting on the device, for the robustness run (split.generate_split(rewrite=...)): a batch's location rows are
// selected out of its canonical graph (csg_graph_rows_select) and rewritten into an equivalent or a corrupted set of rows
// (csg_graph_rewrite); the canonical builder (csg_canon_general_build_dev) makes graphs of both.  The hash and the two row
// rules are csg_rewrite.h's, shared with the host.  No atomics; nothing is read back; every launch is capturable.
#include "csg_bitgraph.h"
#include "csg_common.h"
#include "csg_rewrite.h"

namespace csg {

constexpr int kSelThreads = 256;

struct RewriteIds {
  int pad;
  int pid[6];                                  // __below__ __above__ __left of__ __right of__ __inside__ __surrounding__
};

__device__ __forceinline__ int slot_of(int64_t p, const RewriteIds& ids) {
  int slot = -1;
#pragma unroll
  for (int r = 0; r < 6; ++r) slot = p == (int64_t)ids.pid[r] ? r : slot;
  return slot;
}

__device__ __forceinline__ int pid_of(int slot, const RewriteIds& ids) {
  int pid = ids.pid[0];
#pragma unroll
  for (int r = 1; r < 6; ++r) pid = slot == r ? ids.pid[r] : pid;     // no indexed register: no scratch
  return pid;
}

// One block per sample, the T rows in chunks of 256 in input order.  A chunk's kept rows get their places from a prefix
// sum: a ballot per wave (the rank among the wave's kept rows is a population count), the waves' totals through LDS in
// wave order, the chunks one after the other.  rows[b] = the kept rows, then [0, __padding__, 0]; counts[b] = their
// number, or -1 - it when a location row of type ORIGINAL named an object outside [0, O) and was dropped.
__global__ __launch_bounds__(kSelThreads) void k_graph_rows_select(const int64_t* __restrict__ triplets,
                                                                  const int64_t* __restrict__ triplet_type, int T, int64_t O,
                                                                  RewriteIds ids, int64_t* __restrict__ rows,
                                                                  int64_t* __restrict__ counts) {
  __shared__ int wave_kept[kSelThreads / 64];
  __shared__ int wave_bad[kSelThreads / 64];
  const int b = blockIdx.x, lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int64_t row = (int64_t)b * T;
  int base = 0, bad = 0;
  for (int t0 = 0; t0 < T; t0 += kSelThreads) {
    const int t = t0 + (int)threadIdx.x;
    int64_t s = 0, p = 0, o = 0;
    bool keep = false, dropped = false;
    if (t < T) {
      const int64_t* tr = triplets + (row + t) * 3;
      s = tr[0], p = tr[1], o = tr[2];
      const bool location = slot_of(p, ids) >= 0 && triplet_type[row + t] == 0;
      const bool inside = s >= 0 && s < O && o >= 0 && o < O;
      keep = location && inside;
      dropped = location && !inside;
    }
    const unsigned long long m = __ballot(keep);
    const unsigned long long d = __ballot(dropped);
    if (lane == 0) {
      wave_kept[w] = __popcll(m);
      wave_bad[w] = d != 0ull ? 1 : 0;
    }
    __syncthreads();
    int before = base, total = base;
#pragma unroll
    for (int k = 0; k < kSelThreads / 64; ++k) {
      before += k < w ? wave_kept[k] : 0;
      total += wave_kept[k];
      bad |= wave_bad[k];
    }
    if (keep) {
      const int at = before + __popcll(m & ((1ull << lane) - 1ull));      // at <= t: inside the sample's T rows
      int64_t* out = rows + (row + at) * 3;
      out[0] = s, out[1] = p, out[2] = o;
    }
    base = total;
    __syncthreads();                               // the totals are read before the next chunk writes them
  }
  for (int t = base + (int)threadIdx.x; t < T; t += kSelThreads) {
    int64_t* out = rows + (row + t) * 3;
    out[0] = 0, out[1] = ids.pad, out[2] = 0;
  }
  if (threadIdx.x == 0) counts[b] = bad ? -1 - (int64_t)base : (int64_t)base;
}

// One thread per row of (B,R,3): the first counts[b] rows of a sample go through the mode's rule, every other row (and
// every row of a sample whose count is negative) is copied as it is.  A thread reads its row before it writes it: `out`
// may be `rows`.
__global__ __launch_bounds__(256) void k_graph_rewrite(const int64_t* rows, const int64_t* __restrict__ counts,
                                                       const int64_t* __restrict__ image_id, int64_t n, int R, RewriteIds ids,
                                                       int mode, int direction, uint64_t threshold, uint64_t seed,
                                                       int64_t* out) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int64_t b = i / R;
  const int r = (int)(i - b * R);
  int64_t s = rows[i * 3], p = rows[i * 3 + 1], o = rows[i * 3 + 2];
  int slot = slot_of(p, ids);
  // the hash packs s and o into one word: a row outside [0, 2^31) is no row csg_graph_rows_select left, and is copied
  if (r < counts[b] && slot >= 0 && s >= 0 && s < (1ll << 31) && o >= 0 && o < (1ll << 31)) {
    const uint64_t image = (uint64_t)image_id[b];
    if (mode == CSG_REWRITE_ONE_SIDED)
      rw_one_sided(seed, image, threshold, direction, s, slot, o);
    else
      rw_noise(seed, image, threshold, s, slot, o);
    p = pid_of(slot, ids);
  }
  out[i * 3] = s, out[i * 3 + 1] = p, out[i * 3 + 2] = o;
}

static int rewrite_ids(const char* fn, const int32_t* pred_ids, int64_t P, RewriteIds* ids) {
  CSG_REQUIRE(pred_ids != nullptr, CSG_E_BADSHAPE, "%s: null operand", fn);
  for (int a = 0; a < 8; ++a) {
    CSG_REQUIRE(pred_ids[a] >= 0 && pred_ids[a] < P, CSG_E_BADSHAPE, "%s: predicate id %d outside [0, P = %ld)", fn,
                (int)pred_ids[a], (long)P);
    for (int c = 0; c < a; ++c)
      CSG_REQUIRE(pred_ids[a] != pred_ids[c], CSG_E_BADSHAPE, "%s: the eight predicate ids must be distinct", fn);
    if (a >= 2) ids->pid[a - 2] = pred_ids[a];
  }
  ids->pad = pred_ids[0];
  return CSG_OK;
}

}  // namespace csg

using namespace csg;

extern "C" {

int csg_graph_rows_select(const int64_t* triplets, const int64_t* triplet_type, int64_t B, int64_t T, int64_t O, int64_t P,
                          const int32_t* pred_ids, int64_t* rows, int64_t* counts, void* stream) {
  const char* fn = "csg_graph_rows_select";
  CSG_REQUIRE(B > 0 && B <= 65535 && T >= 0 && T <= (1 << 20) && O > 0 && O <= (1ll << 31) && P > 0 && P <= 4096,
              CSG_E_BADSHAPE, "%s: bad shape B=%ld T=%ld O=%ld P=%ld (B <= 65535, T <= 2^20, O <= 2^31, P <= 4096)", fn, (long)B,
              (long)T, (long)O, (long)P);
  CSG_REQUIRE(counts != nullptr && (T == 0 || (triplets != nullptr && triplet_type != nullptr && rows != nullptr)),
              CSG_E_BADSHAPE, "%s: null operand", fn);
  CSG_REQUIRE(((uintptr_t)triplets | (uintptr_t)triplet_type | (uintptr_t)rows | (uintptr_t)counts) % 8 == 0, CSG_E_BADSHAPE,
              "%s: the int64 operands must be 8-byte aligned", fn);
  CSG_REQUIRE(T == 0 || rows != triplets, CSG_E_BADSHAPE, "%s: rows must not be triplets (a kept row moves ahead of rows unread)",
              fn);
  RewriteIds ids;
  if (const int rc = rewrite_ids(fn, pred_ids, P, &ids)) return rc;
  CSG_LAUNCH(k_graph_rows_select, dim3((unsigned)B), dim3(kSelThreads), 0, (hipStream_t)stream, triplets, triplet_type, (int)T, O,
             ids, rows, counts);
  return check_launch(fn);
}

int csg_graph_rewrite(const int64_t* rows, const int64_t* counts, const int64_t* image_id, int64_t B, int64_t R, int64_t P,
                      const int32_t* pred_ids, int mode, int direction, double share, uint64_t seed, int64_t* out,
                      void* stream) {
  const char* fn = "csg_graph_rewrite";
  CSG_REQUIRE(B > 0 && B <= 65535 && R >= 0 && R <= (1 << 20) && P > 0 && P <= 4096, CSG_E_BADSHAPE,
              "%s: bad shape B=%ld R=%ld P=%ld (B <= 65535, R <= 2^20, P <= 4096)", fn, (long)B, (long)R, (long)P);
  CSG_REQUIRE(share >= 0.0 && share <= 1.0, CSG_E_BADSHAPE, "%s: share %g outside [0, 1]", fn, share);      // a NaN fails both
  CSG_REQUIRE(mode == CSG_REWRITE_ONE_SIDED || mode == CSG_REWRITE_NOISE, CSG_E_BADSHAPE,
              "%s: mode %d is neither one_sided (0) nor noise (1)", fn, mode);
  CSG_REQUIRE(direction == CSG_REWRITE_FORWARD || direction == CSG_REWRITE_BACKWARD || direction == CSG_REWRITE_RANDOM,
              CSG_E_BADSHAPE, "%s: direction %d is none of forward (0), backward (1), random (2)", fn, direction);
  CSG_REQUIRE(counts != nullptr && image_id != nullptr && (R == 0 || (rows != nullptr && out != nullptr)), CSG_E_BADSHAPE,
              "%s: null operand", fn);
  CSG_REQUIRE(((uintptr_t)rows | (uintptr_t)counts | (uintptr_t)image_id | (uintptr_t)out) % 8 == 0, CSG_E_BADSHAPE,
              "%s: the int64 operands must be 8-byte aligned", fn);
  RewriteIds ids;
  if (const int rc = rewrite_ids(fn, pred_ids, P, &ids)) return rc;
  if (R == 0) return CSG_OK;                     // nothing to rewrite, nothing to copy
  const int64_t n = B * R;
  CSG_LAUNCH(k_graph_rewrite, dim3((unsigned)cdiv(n, 256)), dim3(256), 0, (hipStream_t)stream, rows, counts, image_id, n, (int)R,
             ids, mode, direction, rw_threshold(share), seed, out);
  return check_launch(fn);
}

}  // extern "C"
