// Host side of the Winograd kernels (wino.hip, wino4.hip, wino4w.hip), written once: the descriptor check, the split over the
// input channels, the body of a convolution entry point, the weight packs, the slices and the reduction of a weight
// gradient.  Kernels and their launches stay in the file that owns them and come in as callables; nothing here launches a
// kernel of its own (the ordered slab sum is csg_reduce.h's).
#pragma once
#include "csg_common.h"
#include "csg_reduce.h"

namespace csg {

// What every Winograd descriptor has to satisfy: a descriptor, positive dimensions, channel counts and strides in float4
// units, and tensors (and packed weights of `positions` positions, 0: none) inside 32-bit byte offsets.  `pixels(d)` is the
// family's extent: the kernels differ in how far past the last pixel their offsets reach.  The family's own shape rules
// (even / multiple of 4 / whole tile stages, channels per LDS stage) follow this call in its plan.
template <typename Pixels>
static inline int wino_desc_check(const csg_wino_desc* d, const char* who, int positions, Pixels pixels) {
  CSG_REQUIRE(d != nullptr, CSG_E_BADSHAPE, "%s: null descriptor", who);
  CSG_REQUIRE(d->B > 0 && d->H > 0 && d->W > 0 && d->Cin > 0 && d->Cout > 0, CSG_E_BADSHAPE, "%s: non-positive dimension", who);
  CSG_REQUIRE(d->Cin % 4 == 0 && d->x_cs % 4 == 0 && d->x_cs >= d->Cin && d->Cout % 4 == 0 && d->y_cs % 4 == 0 &&
                  d->y_cs >= d->Cout,
              CSG_E_UNSUPPORTED, "%s: channel counts and strides must be multiples of 4", who);
  CSG_REQUIRE((int64_t)pixels(*d) * (int64_t)(d->x_cs > d->y_cs ? d->x_cs : d->y_cs) * 4 < CSG_MAX_RECORDS, CSG_E_UNSUPPORTED,
              "%s: tensor too large for 32-bit byte offsets", who);
  CSG_REQUIRE((int64_t)positions * ((d->Cout + 31) / 32) * ((d->Cin + 7) / 8) * 1024 < CSG_MAX_RECORDS, CSG_E_UNSUPPORTED,
              "%s: packed weights too large for 32-bit byte offsets", who);
  return CSG_OK;
}

// The convolution kernels load x a stage ahead of the channels they use, through a buffer descriptor that spans pixels * x_cs
// floats from x: on a channel slice of a wider tensor that descriptor ends behind the tensor and the prefetch of the last
// pixel would read there.  So the convolution entries take a dense x only; the weight gradients mask their loads at Cin
// and keep x_cs.
static inline int wino_conv_dense_x(const csg_wino_desc* d, const char* who) {
  CSG_REQUIRE(d->x_cs == d->Cin, CSG_E_UNSUPPORTED, "%s: x must be dense (x_cs=%d, Cin=%d)", who, d->x_cs, d->Cin);
  return CSG_OK;
}

// Split over the input channels when the tile grid alone cannot fill the chip (backward-data of the gamma/beta
// convolutions: 128 output channels, 2048 input channels): only without an epilogue (bias / activation / residual / gate)
// and with a dense output; the slabs are summed in a fixed order by k_slab_reduce.  A launch of fewer than 384 blocks is
// cut towards 512, given at least `min_stages` stages in all, into ranges of at least `min_range` stages.
template <typename P>
static inline void wino_split_plan(P& p, bool plain, int min_stages, int min_range) {
  if (!plain || p.y_cs != p.Cout) return;
  const int64_t blocks = (int64_t)p.B * p.tby * p.tbx * p.nblocks;
  if (blocks >= 384 || p.nstage < min_stages) return;
  int ks = (int)((512 + blocks - 1) / blocks);
  if (ks > p.nstage / min_range) ks = p.nstage / min_range;
  if (ks < 2) return;
  p.sps = (p.nstage + ks - 1) / ks;
  p.ksplit = (p.nstage + p.sps - 1) / p.sps;
}

// csg_*_conv_workspace: the slabs of the split a plain launch of this descriptor makes; 0: no split; -1: refused
template <typename P, typename Plan>
static inline int64_t wino_conv_workspace(const csg_wino_desc* d, int min_stages, int min_range, Plan plan) {
  P p;
  size_t shm = 0;
  if (plan(p, shm)) return -1;
  wino_split_plan(p, d->act == CSG_ACT_NONE, min_stages, min_range);
  return p.ksplit > 1 ? (int64_t)p.ksplit * p.slab * 4 : 0;
}

struct WinoConvArgs {       // what the three csg_*_conv entry points are given besides their descriptor
  const float *x, *packed, *bias, *residual, *gate;
  float gate_slope;
  float *y, *workspace;
  int64_t workspace_bytes;
  hipStream_t s;
};

// csg_*_conv: plan -> split -> no slabs: unsplit -> the slabs stand in for y -> alignment -> the family's launch -> the ordered
// slab sum.  `plan(p, shm)` fills the family's parameters, `launch(p, shm, y)` runs its kernel; both report as `who`.  One
// timing scope of `kid` covers the launch and the slab sum; its work is the algorithmic FLOPs of the DIRECT convolution this
// replaces (2 * M * taps*Cin * Cout): what FlopCounterMode counts.
// Alignment: x, packed, the output written (y, or the workspace of a split launch) and, when given, gate must be 16-byte
// aligned — the union of what the three entries used to ask for one by one.
template <typename P, typename Plan, typename Launch>
static inline int wino_conv_entry(const char* who, const char* sum_who, const csg_wino_desc* d, int min_stages, int min_range,
                                  int kid, double taps, const WinoConvArgs& a, Plan plan, Launch launch) {
  P p;
  size_t shm = 0;
  int rc = plan(p, shm);
  if (rc) return rc;
  wino_split_plan(p, d->act == CSG_ACT_NONE && a.bias == nullptr && a.residual == nullptr && a.gate == nullptr, min_stages,
                  min_range);
  p.gate_slope = a.gate_slope;
  if (p.ksplit > 1 && (a.workspace == nullptr || a.workspace_bytes < (int64_t)p.ksplit * p.slab * 4)) {   // no slabs: unsplit
    p.ksplit = 1;
    p.sps = p.nstage;
  }
  float* const y = p.ksplit > 1 ? a.workspace : a.y;
  CSG_REQUIRE(((uintptr_t)a.x % 16) == 0 && ((uintptr_t)a.packed % 16) == 0 && ((uintptr_t)y % 16) == 0 &&
                  (a.gate == nullptr || ((uintptr_t)a.gate % 16) == 0),
              CSG_E_UNSUPPORTED, "%s: x, packed, y, gate and workspace must be 16-byte aligned", who);
  ProfScope ps(kid, 2.0 * (double)(p.slab / p.y_cs) * taps * p.Cin * p.Cout, a.s);
  rc = launch(p, shm, y);
  if (rc == CSG_OK && p.ksplit > 1) {
    launch_slab_reduce(a.workspace, p.slab, a.y, nullptr, 0, nullptr, p.ksplit, a.s);
    rc = check_launch(sum_who);
  }
  return rc;
}

// ---- weight packs: U = G g G^T in the MFMA operand order, `positions` (16 | 36) tables of NT32 x Q8 x 64 lanes x float4
static inline int64_t wino_pack_bytes(int positions, int64_t N, int64_t K) {
  if (N <= 0 || K <= 0) return -1;
  return (int64_t)positions * cdiv(N, 32) * cdiv(K, 8) * 64 * 16;
}

// w is the (Cout, Cin, taps) weight with element strides (s_o, s_i, s_h, s_w) — contiguous or channels-last.
// forward: n = cout, k = cin;  backward-data: n = cin, k = cout, taps flipped.  `launch(grid, stream, kernel arguments...)`
// is the family's: one block of 256 threads per 32 n x 32 k.
template <typename Launch>
static inline int wino_pack_entry(const char* who, int positions, int taps, const float* w, int64_t s_o, int64_t s_i,
                                  int64_t s_h, int64_t s_w, int64_t Cout, int64_t Cin, int32_t backward_data,
                                  const float* sigma, float* packed, void* stream, Launch launch) {
  CSG_REQUIRE(w != nullptr && packed != nullptr && Cout > 0 && Cin > 0, CSG_E_BADSHAPE, "%s: bad arguments", who);
  CSG_REQUIRE(((uintptr_t)packed % 16) == 0, CSG_E_UNSUPPORTED, "%s: packed must be 16-byte aligned", who);
  const int64_t N = backward_data ? Cin : Cout, K = backward_data ? Cout : Cin;
  const int64_t s_n = backward_data ? s_i : s_o, s_k = backward_data ? s_o : s_i;
  const int NT32 = (int)cdiv(N, 32), Q8 = (int)cdiv(K, 8);
  hipStream_t s = (hipStream_t)stream;
  ProfScope ps(K_WINO_PACK, (double)Cout * Cin * taps * 4 + (double)wino_pack_bytes(positions, N, K), s);
  launch(dim3((unsigned)cdiv(Q8, 4), (unsigned)NT32), s, w, s_n, s_k, s_h, s_w, backward_data ? 1 : 0, (int)N, (int)K, sigma, NT32,
         Q8, (float4*)packed);
  return check_launch(who);
}

// ---- weight gradients: the regions of the batch (p.RXn x p.RYn per image) are cut into slices of `tiles2d` blocks each, one
// slab of dW and one row of db per slice (F(3x3,4x4): two).  Aim at `target_blocks` blocks, with at least `min_regions` regions
// per slice and at most `max_slices` slices.
template <typename P>
static inline int wino_wg_slice_plan(P& p, const char* who, int tiles2d, int target_blocks, int min_regions, int max_slices) {
  const int64_t nr = (int64_t)p.B * p.RXn * p.RYn;
  CSG_REQUIRE(nr < (1ll << 30), CSG_E_UNSUPPORTED, "%s: too many regions", who);
  p.nregions = (int)nr;
  int ns = (target_blocks + tiles2d - 1) / tiles2d;
  const int max_ns = (int)((nr + min_regions - 1) / min_regions);
  if (ns > max_ns) ns = max_ns;
  if (ns > max_slices) ns = max_slices;
  if (ns < 1) ns = 1;
  p.rps = (int)((nr + ns - 1) / ns);
  p.nsplit = (int)((nr + p.rps - 1) / p.rps);
  return CSG_OK;
}

// csg_*_bwd_weight_workspace: `nslab` slabs of dW [Cout][3][3][Cin] with their rows of db behind them
static inline int64_t wino_wg_workspace(const csg_wino_desc* d, int nslab) {
  return (int64_t)nslab * d->Cout * (9 * (int64_t)d->Cin + 1) * 4;
}

// The tail of csg_*_bwd_weight: the workspace check, the bias rows behind the weight slabs, the family's
// `launch(slabs, dbslabs)` and the ordered sum into dw / db.  `direct`: a single slab IS the gradient — the kernel writes dw
// and db themselves and nothing is summed (the workspace is still asked for, as csg_*_bwd_weight_workspace sizes it).
template <typename Launch>
static inline int wino_wg_run(const char* who, const char* sum_who, const csg_wino_desc* d, int nslab, bool direct, float* dw,
                              float* db, float* workspace, int64_t workspace_bytes, hipStream_t s, Launch launch) {
  const int64_t wsize = (int64_t)d->Cout * 9 * d->Cin, need = wino_wg_workspace(d, nslab);
  CSG_REQUIRE(workspace != nullptr && workspace_bytes >= need, CSG_E_WORKSPACE, "%s: workspace %ld < %ld bytes", who,
              (long)workspace_bytes, (long)need);
  float* const dbslabs = db != nullptr ? workspace + (int64_t)nslab * wsize : nullptr;
  const int rc = direct ? launch(dw, db) : launch(workspace, dbslabs);
  if (rc || direct) return rc;
  ProfScope ps(K_WGRAD_REDUCE, (double)(nslab + 1) * wsize * 4, s);
  launch_slab_reduce(workspace, wsize, dw, dbslabs, db != nullptr ? d->Cout : 0, db, nslab, s);
  return check_launch(sum_who);
}

}  // namespace csg
