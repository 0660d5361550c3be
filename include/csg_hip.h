/*
 * csg_hip.h — C ABI of libcsg_hip.so: the hand-written gfx950 (MI355X / CDNA4) kernels of the
 * CanonicalSg2Im training hot path.
 *
 * The reference (roeiherz/CanonicalSg2Im) has no FFI of its own: its hot path is PyTorch/ATen
 * calls issued from Python.  Each entry point below therefore replaces one ATen call site of the
 * reference (file:line given per function, relative to the reference root); the Python binding
 * that a maintainer adds on the reference side is the ctypes stub shown in INTEGRATION.md
 * (the build's own binding is canonicalsg2im_amd/_lib.py).
 *
 * Conventions
 *   - plain pointers and sizes only; every pointer is a DEVICE pointer unless marked host.
 *   - the caller allocates every buffer, including workspaces; the library keeps no pointer.
 *   - all work is enqueued on `stream` (a hipStream_t passed as void*); no internal sync,
 *     safe to capture in a hipGraph (profiling mode excepted).
 *   - return 0 on success, a negative CSG_E_* code otherwise; csg_last_error() has the text.
 *     The Python side raises RuntimeError — errors are never swallowed (cf. the reference's
 *     blanket try/except at scripts/train.py:354,440-441, which is NOT reproduced).
 *   - activations are NHWC fp32 ("pixels x channels", channel stride 1); a tensor may be a channel
 *     slice of a wider buffer: `*_cs` is the number of floats per pixel of the underlying buffer.
 *   - indices are int64 as in the reference's collate output (sg2im/data/packed_coco.py:467-478).
 */
#ifndef CSG_HIP_H
#define CSG_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CSG_OK 0
#define CSG_E_BADSHAPE (-1)
#define CSG_E_UNSUPPORTED (-2)
#define CSG_E_LAUNCH (-3)
#define CSG_E_WORKSPACE (-4)

#define CSG_ACT_NONE 0
#define CSG_ACT_LEAKY 1 /* y = x>0 ? x : slope*x ; ReLU is slope 0 */
#define CSG_ACT_TANH 2

#define CSG_MAX_TAPS 16

/* 100 + the number of additive revisions of this header: entry points are only ever added, never changed or removed
 * (108: csg_wino4_conv_spade, csg_wino4_conv_spade_supported, csg_avgpool3s2_bwd_add, csg_hinge_mean_fwd / _bwd;
 * 109: csg_canon_general_workspace, csg_canon_general_build / _converse / _close / _emit;
 * 110: csg_norm_eval_stats_multi, csg_deprocess_u8_workspace, csg_deprocess_u8;
 * 111: csg_box_iou;
 * 112: csg_preprocess_workspace, csg_preprocess;
 * 113: csg_preprocess_px_workspace, csg_preprocess_px, csg_clevr_boxes;
 * 114: csg_vg_rows;
 * 115: csg_draw_boxes_u8; csg_canon_general_build takes boxes = centers = NULL;
 * 116: csg_pair_relations, csg_canon_general_build_dev;
 * 117: csg_canon_small_workspace, csg_canon_small_build, csg_canon_small_emit;
 * 118: csg_clevr_graph_count, csg_clevr_graph_emit;
 * 119: csg_coco_masks;
 * 120: csg_resize_bilinear, csg_pool3, csg_spatial_mean, csg_bias_act, csg_feat_stats, csg_feat_stats_finalize,
 *      csg_softmax_rows, csg_inception_score_workspace, csg_inception_score;
 * 121: csg_draw_labels_u8;
 * 122: csg_draw_graph_u8) */
int csg_version(void);
const char* csg_last_error(void);

/* ---- per-kernel timing (HIP events on the launch stream; used by bench.py's roofline) -------
 * DEVELOPER / BENCHMARK ONLY, and the one piece of MUTABLE PROCESS-GLOBAL STATE in the library (a table of pending event
 * pairs and per-kernel sums behind a mutex, csrc/csg_api.hip): every compute entry point is stateless and re-entrant with
 * the mode off (the default) — apart from immutable once-per-device attributes (raised dynamic-LDS limits) and the
 * thread-local text of csg_last_error().  With a mode on, launches are not graph-capturable and calls from several host
 * threads share one table.
 * mode 0 = off, 1 = every launch, 2 = only the dominant convolution kernels (k_wino4_conv_v, k_wino_conv2<*>, k_igemm_fwd<128>):
 * 3 = only the streaming (HBM-bound) kernels: normalisation, activation, layout, graph gathers, resampling;
 * an event pair costs ~9 us of queue time, 10 ms per step when all ~1100 launches carry one, 2 ms in mode 2. */
int csg_prof_enable(int mode);
int csg_prof_reset(void);
int csg_prof_num_kernels(void);
const char* csg_prof_kernel_name(int kernel_id);
/* synchronises the recorded events; ms = summed launch durations, work = summed algorithmic
 * FLOPs (MFMA-bound kernels) or bytes (HBM-bound kernels) as stated in DESIGN.md */
int csg_prof_read(int kernel_id, double* ms, int64_t* launches, double* work);

/* ---- K1: attribute / predicate embedding lookup ---------------------------------------------
 * replaces nn.Embedding x A + torch.cat (sg2im/attribute_embed.py:40-45) and
 * pred_embeddings (sg2im/model.py:109).
 * out[r, out_off + 0..dim) = table[idx[r*idx_stride], :]                                       */
int csg_embed_fwd(const int64_t* idx, int64_t rows, int64_t idx_stride, const float* table, int64_t num_emb,
                  int64_t dim, float* out, int64_t out_stride, int64_t out_off, void* stream);
/* dtable[idx[r], :] += dout[r, out_off..] — replaces the backward of nn.Embedding (attribute_embed.py:40-45): rows added in
 * row order (no atomics, bit-reproducible).  More than one chunk of 8192 / dim rows needs a workspace of csg_embed_bwd_workspace(...) bytes for
 * the per-chunk partial tables (0 = none needed).
 * LIMITS: dim <= 256 and num_emb * dim < 2^30 (CSG_E_BADSHAPE otherwise; the reference's --embedding_dim is 128).  The
 * workspace is chunks * num_emb * dim floats and the grid re-stages a chunk once per 256 table entries: sized for vocabularies of
 * 10^2..10^3 rows (COCO 184, VG 179 + 46 predicates, CLEVR 4 x <= 9), not for 10^5-row tables.            */
int64_t csg_embed_bwd_workspace(int64_t rows, int64_t num_emb, int64_t dim);
int csg_embed_bwd(const int64_t* idx, int64_t rows, int64_t idx_stride, const float* dout, int64_t out_stride,
                  int64_t out_off, int64_t num_emb, int64_t dim, float* dtable, float* workspace, int64_t workspace_bytes,
                  void* stream);

/* ---- real-object mask: sg2im/utils.py:56-63 (remove_dummy_objects), batched, bit-exact ------ */
int csg_real_object_mask(const int64_t* objs, int64_t B, int64_t O, int64_t A, int64_t image_id, uint8_t* mask,
                         void* stream);

/* ---- K2/K5 support: per-image CSR of triplets by incident object ------------------------------
 * row_ptr (B,O+1) int32, col (B,2T) int32 with col = 2*t + role (role 0 subject, 1 object).
 * Inside a row: all subject entries in t order, then all object entries in t order — the order in
 * which the reference's two scatter_add calls accumulate (sg2im/graph.py:98-99).               */
int csg_graph_csr_build(const int64_t* triplets, int64_t B, int64_t T, int64_t O, int32_t* row_ptr, int32_t* col,
                        void* stream);
/* The builder csg_graph_csr_build launches for (T, O): > 0 = the counting sort (O <= 254, 512 <= T <= 65535) and its
 * dynamic LDS in bytes (at most 150 KB), 0 = the plain builder, -1 = refused.  LIMITS: O <= 1024 objects per image and
 * T < 2^29 (CSG_E_UNSUPPORTED otherwise, before any launch).  Ids outside [0, O) get no entry from either builder. */
int64_t csg_graph_csr_lds(int64_t T, int64_t O);

/* K2: cur_t = cat(obj[s], pred, obj[o])   (sg2im/graph.py:63-66) */
int csg_gather_concat_fwd(const float* obj, const float* pred, const int64_t* triplets, int64_t B, int64_t O,
                          int64_t T, int64_t Din, int64_t Dp, float* out, void* stream);
/* dobj[b,i] = sum over object i's CSR row of the matching slice of dcat; dpred = the middle slice.
 * Dense graphs split each row over several workgroups: the partial sums live in `workspace`
 * (csg_gather_concat_bwd_workspace bytes, 0 for sparse graphs) and are combined in a fixed order.
 * Din and Dp must be multiples of 4 (16-byte rows). */
int64_t csg_gather_concat_bwd_workspace(int64_t B, int64_t O, int64_t T, int64_t Din);
int csg_gather_concat_bwd(const float* dcat, const int32_t* row_ptr, const int32_t* col, int64_t B, int64_t O,
                          int64_t T, int64_t Din, int64_t Dp, float* dobj, float* dpred, void* workspace,
                          int64_t workspace_bytes, void* stream);

/* K4+K5: confidence gate + masked segment average (sg2im/graph.py:69-109).
 * h = net1 output (B,T,2H+Dp) = [s | p | o]; conf (B,T); valid (B,T) = pred_indicators.
 * pooled (B,O,H), cnt (B,O), new_p (B,T,Dp) = conf * h[:, H:H+Dp]
 * H and Dp multiples of 4.  `workspace`: csg_segment_avg_fwd_workspace bytes (row-split partials of
 * dense graphs; 0 for sparse ones).                                                             */
int64_t csg_segment_avg_fwd_workspace(int64_t B, int64_t O, int64_t T, int64_t H);
int csg_segment_avg_fwd(const float* h, const float* conf, const uint8_t* valid, const int32_t* row_ptr,
                        const int32_t* col, int64_t B, int64_t O, int64_t T, int64_t H, int64_t Dp, float* pooled,
                        float* cnt, float* new_p, void* workspace, int64_t workspace_bytes, void* stream);
/* dcnt_scratch (B,O) float workspace.  gate_relu = 1: h is the output of a ReLU (the final non-linearity of net1,
 * sg2im/graph.py:67) and dh is written as the gradient of its PRE-activation (zero where h <= 0): the producing Linear
 * needs no activation-derivative pass. */
int csg_segment_avg_bwd(const float* dpooled, const float* dnew_p, const float* h, const float* conf,
                        const uint8_t* valid, const int64_t* triplets, const float* pooled, const float* cnt,
                        int64_t B, int64_t O, int64_t T, int64_t H, int64_t Dp, int32_t gate_relu, float* dh,
                        float* dconf, float* dcnt_scratch, void* stream);

/* ---- K6: boxes_to_layout (sg2im/layout.py:12-45) and masks_to_layout (:48-77, train mode), batched
 * out[b, y, x, out_off + d] = sum_o valid[b,o] * vecs[b,o,d] * cov(y_src) * cov(x_src)
 * With `masks` (B,O,M,M) fp32 non-NULL the weight of object o at a pixel is the bilinear sample of
 * its mask over the box (grid_sample, align_corners=False, zeros padding) instead of cov*cov.
 * (OH,OW) may be smaller than (H,W): output pixel y samples full-resolution row
 * floor(y*H/OH) — the nearest resize of generator.py:99 / normalization.py:102 folded in.       */
int csg_layout_fwd(const float* vecs, const float* boxes, const uint8_t* valid, const float* masks, int64_t M,
                   int64_t B, int64_t O, int64_t S, int64_t H, int64_t W, int64_t OH, int64_t OW, float* out,
                   int64_t out_cs, int64_t out_off, void* stream);
/* The image discriminator's input `torch.cat([img, layout], dim=1)` (spade/models/networks/discriminator.py:120) built
 * in one pass at full resolution: out (B,H,W,out_cs) NHWC with channels [layout(S) | img(3) | zeros], out_cs >= S + 4 a
 * multiple of 4 (the first convolution's weight is permuted to that order by the caller).  `img` (B,3,H,W) fp32 with
 * element strides (img_sb, img_sc, img_sh, img_sw) — contiguous or channels-last alike.  The layout channels are exactly
 * csg_layout_fwd's.                                                                                                    */
int csg_disc_input_fwd(const float* vecs, const float* boxes, const uint8_t* valid, const float* masks, int64_t M, int64_t B,
                       int64_t O, int64_t S, int64_t H, int64_t W, const float* img, int64_t img_sb, int64_t img_sc,
                       int64_t img_sh, int64_t img_sw, float* out, int64_t out_cs, void* stream);
/* dvecs (B,O,S) = (accumulate ? dvecs : 0) + sum_{y,x} dout * cov * cov.  With `dboxes` (B,O,4) non-NULL (needs
 * `vecs`) the gradient w.r.t. [x0,y0,w,h] is produced too: the grid of layout.py:98-110 is differentiable in the
 * box, and grid_sample's backward w.r.t. its grid is the bilinear weights' derivative.
 * `workspace` (csg_layout_bwd_workspace bytes; 0 when the shape is not served): boxes_to_layout without box gradients
 * on maps from 32 rows up runs as two passes that read dout ONCE — per-tile partial sums for the objects active in the
 * tile, then an ordered sum per object (bit-reproducible).  Without it, one block per (object, image) walks the
 * object's own box support (dout is read once per covering object).                                          */
int64_t csg_layout_bwd_workspace(int64_t B, int64_t O, int64_t S, int64_t OH, int64_t OW, int32_t has_masks,
                                 int32_t box_gradients);
int csg_layout_bwd(const float* dout, int64_t out_cs, int64_t out_off, const float* boxes, const uint8_t* valid,
                   const float* masks, int64_t M, int64_t B, int64_t O, int64_t S, int64_t H, int64_t W, int64_t OH,
                   int64_t OW, float* dvecs, int accumulate, const float* vecs, float* dboxes, void* workspace,
                   int64_t workspace_bytes, void* stream);
/* dmasks (B,O,M,M) = (accumulate ? dmasks : 0) + the gradient of masks_to_layout (layout.py:48-77) w.r.t. the masks:
 * grid_sample's backward w.r.t. its input, summed over the embedding channels (dout . vecs per pixel).  One block per
 * (object, image), every mask cell an ordered sum.  Rows of invalid objects are zero.                         */
int csg_layout_bwd_masks(const float* dout, int64_t out_cs, int64_t out_off, const float* boxes, const uint8_t* valid,
                         int64_t M, int64_t B, int64_t O, int64_t S, int64_t H, int64_t W, int64_t OH, int64_t OW,
                         const float* vecs, float* dmasks, int accumulate, void* stream);
/* masks_to_layout(test_mode=True) (layout.py:71-74,135-151): painter's compositing, one object per pixel.
 * csg_layout_mass: mass[b,o] = sum(samples[o]) at full resolution (+inf for invalid objects) — the caller sorts it
 * (ascending, stable) into `order` (B,O) int32, -1 after the last valid object.
 * csg_layout_paint: pixel -> first object of `order` whose sampled mask is > 0.5, value vec * mask sample.  */
int csg_layout_mass(const float* vecs, const float* boxes, const uint8_t* valid, const float* masks, int64_t M,
                    int64_t B, int64_t O, int64_t S, int64_t H, int64_t W, float* mass, void* stream);
int csg_layout_paint(const float* vecs, const float* boxes, const float* masks, int64_t M, const int32_t* order,
                     int64_t B, int64_t O, int64_t S, int64_t H, int64_t W, int64_t OH, int64_t OW, float* out,
                     int64_t out_cs, int64_t out_off, void* stream);

/* ---- K3/K8/K11: implicit-GEMM convolution on fp32 MFMA ---------------------------------------
 * replaces nn.Conv2d (generator.py:28,46; architecture.py:29-32; normalization.py:89-94;
 * discriminator.py:175-187) and nn.Linear (sg2im/layers.py:10; a Linear is a 1x1 conv on an
 * (M,1,1,K) image).  One descriptor covers forward, backward-data (transposed taps, weights packed
 * [Cin][tap][Cout]) and the parity classes of a stride-2 transposed convolution.
 *
 * GEMM view: rows m = (b, gy, gx) over the output grid, cols n = output channel,
 * k = (tap slot, input channel).  Virtual input coordinate of tap t for grid point (gy,gx):
 *   iy = gy*istride + tap_dy[t], ix = gx*istride + tap_dx[t]; outside [0,IHv)x[0,IWv) reads 0;
 *   the physical source pixel is (iy >> in_up, ix >> in_up) (nearest 2x upsample folded in).
 * Packed weights: w[n][tap_w[t]][c], c fastest, row length wtaps*Cin.
 * Output pixel of grid point: (gy*os + ooy, gx*os + oox) in an (OHf,OWf) image.
 * res_gate = 1: `residual` is not added but GATES the result, y = result * (residual > 0 ? 1 : slope) — the derivative
 * of the (Leaky)ReLU whose output `residual` is: a backward-data pass hands the producer of its input the gradient of the
 * PRE-activation and no separate activation-derivative pass runs.  Requires act == CSG_ACT_NONE (slope is then the
 * gate's negative slope).                                                                                            */
typedef struct csg_conv_desc {
  int32_t B, IHp, IWp, Cin, x_cs;
  int32_t IHv, IWv, in_up;
  int32_t OHg, OWg, OHf, OWf, os, ooy, oox;
  int32_t Cout, y_cs;
  int32_t istride, ntaps, wtaps;
  int32_t tap_dy[CSG_MAX_TAPS], tap_dx[CSG_MAX_TAPS], tap_w[CSG_MAX_TAPS];
  int32_t act;
  float slope;
  int32_t accumulate; /* y += result (after bias/act) instead of y = */
  int32_t res_gate; /* 1: the residual gates the result instead of being added (see above) */
} csg_conv_desc;

/* y = act(conv(x, w) + bias) [+ residual];  bias and residual may be NULL; residual has y's layout.
 * Layers whose output grid is too small to fill 256 CUs are split along K into `workspace` slabs
 * that an ordered second pass sums (csg_conv_fwd_workspace bytes; a NULL/short workspace when that is non-zero
 * is CSG_E_WORKSPACE, as for the multi and weight-gradient entry points). */
int64_t csg_conv_fwd_workspace(const csg_conv_desc* d);
int csg_conv_fwd(const csg_conv_desc* d, const float* x, const float* w, const float* bias, const float* residual,
                 float* y, float* workspace, int64_t workspace_bytes, void* stream);
/* Up to four descriptors that share weights, input, output tensor, channel counts and batch, served by ONE launch: the
 * parity classes of a stride-2 transposed convolution (backward-data of the PatchGAN's 4x4/2 layers,
 * discriminator.py:175-183).  Each class alone fills a fraction of the chip.  Workspace as csg_conv_fwd's.        */
int64_t csg_conv_fwd_multi_workspace(const csg_conv_desc* descs, int32_t n);
int csg_conv_fwd_multi(const csg_conv_desc* descs, int32_t n, const float* x, const float* w, const float* bias,
                       const float* residual, float* y, float* workspace, int64_t workspace_bytes, void* stream);
/* dw[n][tap][c] = sum_m dy[m][n] * x[src(m,tap)][c]; `d` is the FORWARD descriptor (y_cs = floats per
 * pixel of dy).  Deterministic split-K: partial slabs in `workspace`, then an ordered reduction.
 * db (Cout floats, may be NULL) receives the bias gradient sum_m dy[m][n], accumulated from the dY
 * tiles the kernel stages anyway (no separate pass over dy). */
int64_t csg_conv_bwd_weight_workspace(const csg_conv_desc* d);
int csg_conv_bwd_weight(const csg_conv_desc* d, const float* x, const float* dy, float* dw, float* db,
                        float* workspace, int64_t workspace_bytes, void* stream);

/* ---- K8w: 3x3 / stride 1 / pad 1 convolution by Winograd F(2x2,3x3) on fp32 MFMA (csrc/wino.hip) ----
 * The same nn.Conv2d call sites as above restricted to 3x3 kernels (generator.py:28; architecture.py:29-31;
 * normalization.py:89-94) and their backward-data passes: 16 instead of 36 multiplications per 2x2 output tile
 * and (cin,cout) pair, fp32 throughout.  x (B,H,W,Cin) NHWC, dense: every convolution entry of the Winograd families
 * (csg_wino_conv, csg_wino4_conv, _conv_part, _conv_spade, csg_wino34_conv) refuses x_cs != Cin with CSG_E_UNSUPPORTED —
 * the kernels load x a stage ahead through a descriptor of pixels * x_cs floats, which on a channel slice would end behind
 * the tensor; the weight gradients below take x with channel stride x_cs.  y (and residual, gate) with channel stride y_cs;
 * H, W even; channel counts multiples of 4.  y = act(conv + bias) [+ residual] exactly as csg_conv_fwd.
 * `packed`: the transformed weights U = G g G^T in MFMA operand order, csg_wino_pack_bytes(N, K) bytes, produced by
 * csg_wino_pack_weights from the (Cout,Cin,3,3) weight with element strides (s_o,s_i,s_h,s_w) — contiguous or
 * channels-last parameters alike: backward_data = 0 -> operand of the forward
 * (N = Cout, K = Cin); 1 -> operand of dX = conv(dY, flipped W^T) (N = Cin, K = Cout: call csg_wino_conv with
 * Cin := Cout, Cout := Cin).  `sigma` (device scalar or NULL) divides every weight first — W / sigma of spectral
 * normalisation — so a spectrally normalised layer needs no materialised W_eff.                            */
typedef struct csg_wino_desc {
  int32_t B, H, W;
  int32_t Cin, x_cs;
  int32_t Cout, y_cs;
  int32_t act;
  float slope;
} csg_wino_desc;
int64_t csg_wino_pack_bytes(int64_t N, int64_t K);
int csg_wino_pack_weights(const float* w, int64_t s_o, int64_t s_i, int64_t s_h, int64_t s_w, int64_t Cout, int64_t Cin,
                          int32_t backward_data, const float* sigma, float* packed, void* stream);
/* `workspace` (csg_wino_conv_workspace(d) bytes, may be 0 / NULL): slabs of a split over the input channels, used
 * when the tile grid alone cannot fill the chip and the call has no epilogue (bias, residual, activation) — the
 * backward-data pass of the 128 -> 2048 gamma/beta convolutions; summed in a fixed order (bit-reproducible).
 * Without (enough) workspace the launch runs unsplit.
 * `gate` (nullable, the layout of y): y *= (gate > 0 ? 1 : gate_slope) as the last step — the derivative of the
 * (Leaky)ReLU that PRODUCED this convolution's input, folded into the backward-data pass of the SPADE gamma/beta
 * convolutions (their input `actv` = ReLU(mlp_shared(seg)), normalization.py:96-100, has no other consumer), which
 * replaces a separate pass over the 128-channel maps.  A gated call is never split.                              */
int64_t csg_wino_conv_workspace(const csg_wino_desc* d);
int csg_wino_conv(const csg_wino_desc* d, const float* x, const float* packed, const float* bias,
                  const float* residual, const float* gate, float gate_slope, float* y, float* workspace,
                  int64_t workspace_bytes, void* stream);
/* Weight gradient of the same layers by Winograd F(3x3,2x2): dw [Cout][3][3][Cin] (the layout of
 * csg_conv_bwd_weight), db (Cout) or NULL; x (B,H,W,Cin) the layer's input with channel stride x_cs, dy (B,H,W,Cout) the
 * gradient of its pre-activation output with channel stride y_cs.  Deterministic: per-slice slabs in `workspace` + an ordered reduction.              */
int64_t csg_wino_bwd_weight_workspace(const csg_wino_desc* d);
int csg_wino_bwd_weight(const csg_wino_desc* d, const float* x, const float* dy, float* dw, float* db, float* workspace,
                        int64_t workspace_bytes, void* stream);

/* Weight gradient of the same layers by Winograd F(3x3,4x4) (csrc/wino4w.hip): 36 multiplications per 4x4 tile of dY where
 * F(3x3,2x2) needs 64 — the layers of architecture.py:29-31 and normalization.py:89-94 on maps whose H and W are multiples
 * of 8 (efficient from 64 input and 64 output channels up: a block owns 64 x 64 channels).  Same arguments, layouts and
 * determinism as csg_wino_bwd_weight; csg_wino4_bwd_weight_workspace < 0: the shape is not served.                   */
int64_t csg_wino4_bwd_weight_workspace(const csg_wino_desc* d);
int csg_wino4_bwd_weight(const csg_wino_desc* d, const float* x, const float* dy, float* dw, float* db, float* workspace,
                         int64_t workspace_bytes, void* stream);

/* ---- K8w4: the same 3x3 / stride 1 / pad 1 layers by Winograd F(4x4,3x3) (csrc/wino4.hip) ------------------------
 * 36 multiplications per 4x4 output tile and (cin,cout) pair — 2.25 per output where F(2x2,3x3) needs 4 — on maps at
 * least 32 pixels wide (H, W multiples of 4, H >= 16, Cin a multiple of 8); interpolation points {0, 1, -1, 1/2, -2,
 * inf}, error against fp64 < 1e-5 of the output scale (tests/test_gpu_wino4.py).  Same descriptor, arguments and
 * epilogue as csg_wino_conv; the packed operand has 36 positions (csg_wino4_pack_bytes / csg_wino4_pack_weights, same
 * arguments as the F(2x2,3x3) pack).  csg_wino4_supported(d) = 1 when a layer is served (0 also when CSG_WINO4=0).   */
int32_t csg_wino4_supported(const csg_wino_desc* d);
/* Several (Cout,Cin,3,3) weights packed by ONE launch per kernel family and 24 items: a pack costs ~7 us of fixed latency
 * whatever its size (tools/pack_bench.py) and a generator step needs about a hundred.  Each item is what
 * csg_wino_pack_weights (variant 2, F(2x2,3x3)) / csg_wino4_pack_weights (variant 4, F(4x4,3x3)) take, without the
 * spectral-norm divisor; outputs are bit-identical to the one-weight calls.  `items` is host memory, read during the
 * call (the table travels in the kernel arguments: the launch can be captured in a HIP graph).                        */
typedef struct csg_wino_pack_item {
  const float* w;            /* (Cout,Cin,3,3) with element strides s_o, s_i, s_h, s_w */
  int64_t s_o, s_i, s_h, s_w;
  int64_t Cout, Cin;
  int32_t backward_data;     /* 1: the operand of the backward-data pass (channel roles swapped, taps flipped) */
  int32_t variant;           /* 2 | 4 */
  float* packed;             /* csg_wino_pack_bytes / csg_wino4_pack_bytes (N, K) bytes, 16-byte aligned */
} csg_wino_pack_item;
int csg_wino_pack_weights_multi(const csg_wino_pack_item* items, int32_t n, void* stream);
/* Launches with at least two (region, 64-channel block) items per CU, an even number of 8-channel stages (>= 4) and
 * Cout a multiple of 64 run as ONE block per CU that walks its items with the stage pipeline carried across them
 * (bit-identical outputs).  csg_wino4_persistent(0 | 1) switches that form off / on for the process
 * and returns the previous setting (-1 = not yet decided: CSG_WINO4_PERSIST, default 1); a negative argument only
 * queries.  For A/B measurements and the parity tests — not needed in normal use.                                    */
int32_t csg_wino4_persistent(int32_t on);
int64_t csg_wino4_pack_bytes(int64_t N, int64_t K);
int csg_wino4_pack_weights(const float* w, int64_t s_o, int64_t s_i, int64_t s_h, int64_t s_w, int64_t Cout, int64_t Cin,
                           int32_t backward_data, const float* sigma, float* packed, void* stream);
int64_t csg_wino4_conv_workspace(const csg_wino_desc* d);
int csg_wino4_conv(const csg_wino_desc* d, const float* x, const float* packed, const float* bias,
                   const float* residual, const float* gate, float gate_slope, float* y, float* workspace,
                   int64_t workspace_bytes, void* stream);

/* A slice of the outputs of an F(4x4,3x3) convolution — 32-channel tiles [tile_off, tile_off + Cout/32) of a packed
 * operand of `tiles_total` tiles — optionally with the SPADE modulation (normalization.py:96-110) as its epilogue:
 * with mod_x != NULL the launch is the BETA half of the gamma || beta convolution and writes
 *     y = leaky(((mod_x - mean) * invstd) * (1 + gamma) + (conv + bias), mod_slope)
 * where `mod_gamma` (pixel stride gamma_cs) is the gamma map a plain launch of this entry point (tile_off 0, y_cs =
 * gamma_cs) wrote before, mod_x has y's layout and mean / invstd are the (C,) batch statistics.  beta never reaches
 * memory and the apply pass of csg_norm_apply_fwd is not needed.  `bias` points at the slice's first channel.      */
int csg_wino4_conv_part(const csg_wino_desc* d, const float* x, const float* packed, int64_t tile_off, int64_t tiles_total,
                        const float* bias, const float* mod_x, const float* mod_gamma, int64_t gamma_cs,
                        const float* mod_mean, const float* mod_invstd, float mod_slope, float* y, void* stream);

/* ONE launch for a SPADE modulation (normalization.py:89-110; round 6): the gamma || beta convolution (`packed`: the ordinary
 * F(4x4,3x3) forward operand of the (2C, Cin, 3, 3) weight, gamma tiles then beta tiles; `bias`: its 2C biases) with
 *     y = leaky(((mod_x - mean) * invstd) * (1 + gamma) + beta, mod_slope)
 * as the epilogue of blocks that own a gamma tile and the beta tile of the same 32 channels.  d->Cout = C (the modulated map's
 * channels, a multiple of 32), y and mod_x are (B,H,W,y_cs).  `gamma_out` (nullable; pixel stride gamma_cs): gamma = conv +
 * bias is also written there — the backward reads it (csg_norm_apply_bwd_reduce / _dx); inference passes NULL.  beta never
 * reaches memory.  Outputs are bit-identical to csg_wino4_conv_part(gamma) followed by csg_wino4_conv_part(beta).
 * Served by the persistent form of the kernel only: csg_wino4_conv_spade_supported(d) = 1 when the launch has at least two
 * (region, 32-channel gamma + beta block) items per CU and an even number (>= 4) of 8-channel stages; else the launch pair. */
int32_t csg_wino4_conv_spade_supported(const csg_wino_desc* d);
int csg_wino4_conv_spade(const csg_wino_desc* d, const float* x, const float* packed, const float* bias, const float* mod_x,
                         float* gamma_out, int64_t gamma_cs, const float* mod_mean, const float* mod_invstd, float mod_slope,
                         float* y, void* stream);

/* ---- K8w34: 4x4 / stride 1 convolutions by Winograd F(3x3,4x4) (csrc/wino4.hip, the same kernel on 3x3 output tiles)
 * The PatchGAN's fourth layer (discriminator.py:184-189: 4x4, stride 1, padding 2, 256 -> 512 channels at 1/8
 * resolution) and its backward-data pass (the 4x4 correlation with the flipped, transposed weight and padding 1):
 * 36 multiplications per 3x3 output tile instead of 144.  d->H, d->W are the INPUT size; `pad` is 2 (output (H+1) x
 * (W+1)) or 1 (output (H-1) x (W-1)); x (B,H,W,x_cs), y (B,Ho,Wo,y_cs), residual / gate in y's layout.  Same points,
 * input transform and positions as F(4x4,3x3): the packed operand has csg_wino4_pack_bytes bytes.                    */
int32_t csg_wino34_supported(const csg_wino_desc* d, int32_t pad);
int csg_wino34_pack_weights(const float* w, int64_t s_o, int64_t s_i, int64_t s_h, int64_t s_w, int64_t Cout, int64_t Cin,
                            int32_t backward_data, const float* sigma, float* packed, void* stream);
/* `workspace` (csg_wino34_conv_workspace bytes, may be 0 / NULL) as csg_wino_conv's: slabs of a split over the input
 * channels when the tile grid alone cannot fill the chip (the half-resolution scale's backward-data pass: 128 blocks)
 * and the call has no epilogue; summed in a fixed order.                                                        */
int64_t csg_wino34_conv_workspace(const csg_wino_desc* d, int32_t pad);
int csg_wino34_conv(const csg_wino_desc* d, int32_t pad, const float* x, const float* packed, const float* bias,
                    const float* residual, const float* gate, float gate_slope, float* y, float* workspace,
                    int64_t workspace_bytes, void* stream);

/* ---- K8n: stride-1 convolutions with at most four output channels (csrc/fewn.hip) --------------------------------
 * `conv_img` (generator.py:46,120-121: 64 -> 3, 3x3, pad 1, tanh behind it) and the PatchGAN prediction heads
 * (discriminator.py:185-187: 512 -> 1, 4x4, pad 2): a 32-wide MFMA tile wastes 29 (31) of its columns on them; these
 * are VALU kernels that move the many-channel side once.  Output channels are padded to 4 (y, dy: (B,OH,OW,4); w, dw:
 * [4][KH][KW][Cin]; the forward and backward-data passes read only the first cout_real rows of w and entries of bias,
 * the weight gradient writes all four rows of dw / entries of db, zeros beyond cout_real); KH = KW in {3, 4}; Cin in {32, 64, ..., 1024};
 * KH*KW*cout_real <= 36.  The weight gradient is bit-reproducible (per-block slabs + ordered sum).               */
typedef struct csg_few_desc {
  int32_t B, IH, IW;
  int32_t Cin, x_cs;
  int32_t KH, KW, pad;
  int32_t cout_real;
  int32_t act;
  float slope;
  int32_t in_act; /* 1: the convolution sees leaky(x, in_slope): the LeakyReLU in front of conv_img (generator.py:123-124) is
                   * applied in the forward and weight-gradient loaders instead of a pass of its own; backward-data callers
                   * multiply by its derivative themselves (csg_conv_desc.res_gate) */
  float in_slope;
} csg_few_desc;
int csg_conv_few_supported(const csg_few_desc* d);      /* 1 / 0 */
/* forward `workspace` (csg_conv_few_fwd_workspace bytes, may be 0): slabs of a split over the input channels for maps
 * with few pixels and many channels (the heads); summed in a fixed order.  Without it the launch runs unsplit.    */
int64_t csg_conv_few_fwd_workspace(const csg_few_desc* d);
int csg_conv_few_fwd(const csg_few_desc* d, const float* x, const float* w, const float* bias, float* y, float* workspace,
                     int64_t workspace_bytes, void* stream);
int csg_conv_few_bwd_data(const csg_few_desc* d, const float* dy, const float* w, float* dx, void* stream);
int64_t csg_conv_few_bwd_weight_workspace(const csg_few_desc* d);
int csg_conv_few_bwd_weight(const csg_few_desc* d, const float* x, const float* dy, float* dw, float* db,
                            float* workspace, int64_t workspace_bytes, void* stream);

/* ---- plain fp32 GEMMs (csrc/gemm.hip) ------------------------------------------------------------
 * The layers of the path that ARE matrix products: nn.Linear of the graph encoder (sg2im/graph.py:63-77 through
 * sg2im/layers.py:114-140 build_mlp; rows = triplets or objects) and 1x1 convolutions on NHWC maps (SPADEResnetBlock.conv_s,
 * spade/models/networks/architecture.py:37-39; rows = pixels).  csg_conv_fwd / csg_conv_bwd_weight serve them as well (the
 * small ones stay there); these kernels drop the convolution's tap table and stage both operands by LDS-DMA.
 *   csg_gemm_nt:  y[m][n] = epi(sum_k a[m][k] * bw[n][k] + bias[n]);  epi = act, then `gate` (nullable, rows of ldg
 *                 floats): y *= (gate[m][n] > 0 ? 1 : gate_slope) — the derivative of the (Leaky)ReLU that produced this
 *                 layer's input, for the backward-data pass (a = dy, bw = W^T stored [K_layer][N_layer]).
 *   csg_gemm_tn:  dw[n][k] = sum_m dy[m][n] * x[m][k]  ([Cout][Cin] = the layout of csg_conv_bwd_weight for a 1x1
 *                 filter), db[n] = sum_m dy[m][n] (nullable).  Rows are cut into slices with one slab each in `workspace`
 *                 (csg_gemm_tn_workspace bytes, 0 = none needed), summed in a fixed order: bit-reproducible.
 * K, N (tn), every row stride: multiples of 4 floats; pointers 16-byte aligned.                                       */
typedef struct csg_gemm_desc {
  int64_t M, N, K;
  int64_t lda, ldb, ldy, ldg; /* floats per row of a, bw, y, gate */
  int32_t act;                /* CSG_ACT_NONE / CSG_ACT_LEAKY (ReLU = slope 0) */
  float slope;
  float gate_slope;
} csg_gemm_desc;
int csg_gemm_supported(const csg_gemm_desc* d);
int csg_gemm_nt(const csg_gemm_desc* d, const float* a, const float* bw, const float* bias, const float* gate, float* y,
                void* stream);
int64_t csg_gemm_tn_workspace(int64_t M, int64_t N, int64_t K);
int csg_gemm_tn(int64_t M, int64_t N, int64_t K, const float* dy, int64_t ldy, const float* x, int64_t ldx, float* dw,
                float* db, float* workspace, int64_t workspace_bytes, void* stream);

/* dpre = dy * act'(.) evaluated from the OUTPUT y (leaky: y>0 ? 1 : slope; tanh: 1-y^2)          */
int csg_act_bwd(const float* dy, const float* y, int64_t n, int32_t act, float slope, float* dpre, void* stream);
/* out[c] = sum_rows x[r, c] over (rows, C) with row stride x_cs — bias gradients; partial (nchunk,2C) fp64 */
int csg_colsum(const float* x, int64_t rows, int64_t C, int64_t x_cs, float* out, double* partial, int64_t nchunk,
               void* stream);

/* ---- K9/K11: BatchNorm / InstanceNorm statistics + SPADE modulation + LeakyReLU ---------------
 * replaces F.batch_norm (sync_batchnorm/batchnorm.py:65-68), the modulation of
 * normalization.py:108, F.leaky_relu (architecture.py:53-54,67-68) and nn.InstanceNorm2d +
 * LeakyReLU (normalization.py:44, discriminator.py:181-185).
 * x is (G groups, P pixels, C channels): BatchNorm G=1, P=B*h*w; InstanceNorm G=B, P=h*w.
 * sums (G,2C) double = [sum x | sum x^2]; it is the message SyncBN all-reduces
 * (batchnorm.py:74-83).  Accumulated in fp64 throughout (partial: (G,nchunk,2C) doubles): x and x*x are
 * exact in fp64, so E[x^2]-E[x]^2 loses nothing to the chunking.                                 */
int csg_norm_stats(const float* x, int64_t G, int64_t P, int64_t C, double* sums, double* partial, int64_t nchunk,
                   void* stream);
/* mode 0: invstd = 1/sqrt(var+eps) (F.batch_norm); mode 1: invstd = clamp(var,eps)^-1/2
 * (batchnorm.py:145, N-replica path).  running_* may be NULL; running_var gets the unbiased var. */
int csg_norm_finalize(const double* sums, int64_t G, int64_t C, double count, float eps, int32_t mode, float* mean,
                      float* invstd, float* running_mean, float* running_var, float momentum, void* stream);
/* One-rank statistics in two launches instead of three: csg_norm_stats's first stage, then ONE kernel that reduces the
 * partial table (the same fixed order: bit-identical sums) and finalises as csg_norm_finalize does with mode 0 — mean,
 * invstd = (var + eps)^-1/2 and the running statistics of up to two modules that see the same batch (norm_0 and norm_s of
 * a SPADE residual block, architecture.py:37-47).  Not for N > 1 ranks: there the sums travel between the two steps. */
int csg_norm_stats_finalize(const float* x, int64_t G, int64_t P, int64_t C, double* partial, int64_t nchunk, double count,
                            float eps, float* mean, float* invstd, float* running_mean, float* running_var,
                            float* running_mean2, float* running_var2, float momentum, void* stream);
/* y = leaky((x-mean)*invstd*(1+gamma)+beta, slope); gb (G*P, 2C) = [gamma | beta] or NULL; slope 1 = no act.
 * (gb2, slope2, y2), nullable: a second modulation of the same normalised x written in the same pass.           */
int csg_norm_apply_fwd(const float* x, const float* mean, const float* invstd, const float* gb, float slope,
                       int64_t G, int64_t P, int64_t C, float* y, const float* gb2, float slope2, float* y2,
                       void* stream);
/* Eval-mode statistics of MANY BatchNorms in one launch (F.batch_norm(training=False), sync_batchnorm/batchnorm.py:65-68, for
 * every param-free norm of the generator's SPADE layers, normalization.py:100): item i turns its (running_mean, running_var)
 * into out[offset, offset + C) = mean and out[offset + C, offset + 2C) = invstd = 1 / sqrt(var + eps) — fp32, correctly rounded
 * square root and division (the one-device formula, not the N-replica clamp).  What csg_norm_apply_fwd, csg_wino4_conv_part and
 * csg_wino4_conv_spade take as (mean, invstd) at inference: computed once per loaded checkpoint, not per call.  `items` is
 * host memory read during the call (the table travels in the kernel arguments, 32 items per launch); the slots must not
 * overlap and come in ascending order; offsets that are multiples of 4 keep the vectors 16-byte aligned.              */
typedef struct csg_norm_eval_item {
  const float* running_mean;
  const float* running_var;
  int64_t C;
  int64_t offset;            /* in floats, into `out` */
} csg_norm_eval_item;
int csg_norm_eval_stats_multi(const csg_norm_eval_item* items, int32_t n, float eps, float* out, void* stream);
/* pass 1: dgb (if gb; always (G*P, 2C) = [d gamma | d beta]) and dsums (G,2C) double = [sum dn | sum dn*xhat].  `yact`
 * (nullable, with gb): the activated output y of the forward — the LeakyReLU gate is then read off y's sign and beta is
 * never read; gb may then be a gamma-only map.  `gb_cs`: floats per pixel of gb — 2C ([gamma | beta]) or, with yact, C
 * (what the fused forward csg_wino4_conv_part keeps: it never materialises beta).                                  */
int csg_norm_apply_bwd_reduce(const float* dy, const float* x, const float* mean, const float* invstd,
                              const float* gb, const float* yact, float slope, int64_t G, int64_t P, int64_t C, float* dgb,
                              double* dsums, double* partial, int64_t nchunk, int64_t gb_cs, void* stream);
/* pass 2: dx = invstd*(dn - dsum0/count - xhat*dsum1/count).  (dy2, gb2, slope2), nullable: a second SPADE modulation
 * of the SAME normalised x (norm_0 and norm_s of a residual block with a learned shortcut, architecture.py:37-47, see
 * the same batch statistics): dn = dn_1 + dn_2 and `dsums` holds the sum of both pass-1 reductions — one pass and one
 * dx instead of two passes and an addition.  `dgb` / `dgb2` (nullable): pass 1's output for the same modulation — its
 * d(beta) half IS dy times the activation gate, so pass 2 reads it instead of dy and beta (one map less, same bits).
 * `gb_cs`: floats per pixel of gb and gb2 — 2C, or C for gamma-only maps (then dgb / dgb2 are required).             */
int csg_norm_apply_bwd_dx(const float* dy, const float* x, const float* mean, const float* invstd, const float* gb,
                          float slope, const double* dsums, double count, int64_t G, int64_t P, int64_t C, float* dx,
                          const float* dy2, const float* gb2, float slope2, const float* dgb, const float* dgb2,
                          int64_t gb_cs, void* stream);

/* ---- generated image -> uint8 picture (csrc/deprocess.hip) ------------------------------------------
 * deprocess_batch(imgs, rescale, imagenet_deprocess) (sg2im/data/utils.py:36-65) on the device, with the reference's order of
 * fp32 operations per element (T.Normalize is sub_(mean).div_(std)):
 *   t = x / div3[c]  (:38, INV_IMAGENET_STD);  t = t - sub3[c]  (:39, INV_IMAGENET_MEAN);
 *   rescale: t = (t - lo_b) / (hi_b - lo_b) with lo_b, hi_b = min, max over the whole image b after the two steps (:31-33);
 *   out = byte(clamp(t * 255, 0, 255))  (:62, truncation).
 * No multiply-add is contracted and the divisions are correctly rounded: the bytes EQUAL those of the fp32 host code.
 * img (B,H,W,img_cs) NHWC fp32, img_cs 3 or 4 (channels-last 3-channel image, or conv_img's 4-padded output), W a multiple
 * of 4; out (B,3,H,W) uint8 planar; div3 / sub3: three floats each, HOST memory, read during the call.  Two launches with
 * rescale (per-image min / max partials in `workspace`, csg_deprocess_u8_workspace(B) bytes — ordered trees, no atomics,
 * NaN propagates as in torch.min / max), one without (workspace may be NULL).
 * An image with hi_b == lo_b (constant, or one holding a NaN) makes every element NaN in the reference's arithmetic, and
 * byte() of a NaN is undefined in C++; this entry point writes 0, what torch's x86 host kernels produce
 * (tests/test_gpu_sample.py pins that against torch on the host).  The case cannot be refused with an error code without
 * a device synchronisation, which the capturable-launch convention above rules out.                              */
int64_t csg_deprocess_u8_workspace(int64_t B);
int csg_deprocess_u8(const float* img, int64_t B, int64_t H, int64_t W, int64_t img_cs, const float* div3, const float* sub3,
                     int32_t rescale, uint8_t* out, float* workspace, int64_t workspace_bytes, void* stream);

/* ---- box outlines on a uint8 picture (csrc/overlay.hip) -------------------------------------------------
 * The layout picture of scripts/run_model.py (the generated image with the predicted boxes on it, sg2im/vis.py:128-146)
 * without text labels.  img (B,3,H,W) uint8 planar as csg_deprocess_u8 writes it, W a multiple of 4; boxes (B,O,4) fp32
 * xywh; objs (B,O,A) int64 (attribute 0 is read); palette (P,3) uint8 RGB; out (B,3,H,W) uint8, another buffer than img,
 * which is only read.  All device memory.
 * Row o of sample b is skipped when objs[b,o,0] == image_id, when all four box values are -1, when one of them is NaN, or
 * when w <= 0 or h <= 0.  For the others, in fp32 and in this order (no multiply-add is contracted):
 *   x0 = clamp(x, 0, 1), x1 = clamp(x + w, 0, 1), likewise y  (the clamp of a NaN sum, -inf + inf, is 0);
 *   px0 = min(W - 1, (int)(x0 * W)), px1 = max(px0, min(W - 1, (int)(x1 * W) - 1)), likewise y with H.
 * A pixel is on row o's outline when it lies in [px0, px1] x [py0, py1] and its distance to the nearest side of that
 * rectangle is < thickness (>= 1).  A pixel on no outline keeps its byte; one on several takes palette[o % P] of the
 * HIGHEST such o.  One launch, capturable, nothing is read back; each lane decides its own pixels, so the bytes are the
 * same on every run.
 * LIMITS: 1 <= B <= 65535; O <= 256 and P <= 256 (CSG_E_UNSUPPORTED beyond); H * W < 2^31; img and out on a 4-byte
 * boundary, boxes on a 16-byte one.
 * The boxes' names are drawn by csg_draw_labels_u8 below, on the picture this entry point returns.                  */
int csg_draw_boxes_u8(const uint8_t* img, const float* boxes, const int64_t* objs, int64_t B, int64_t O, int64_t A, int64_t H,
                      int64_t W, int64_t image_id, const uint8_t* palette, int64_t P, int32_t thickness, uint8_t* out,
                      void* stream);

/* ---- the boxes' names on a uint8 picture (csrc/overlay.hip) ---------------------------------------------
 * The coloured strip with the object's name that sg2im/vis.py:16-41 puts across the top of each box, in a 5 x 7 font.
 * img, boxes, objs, B, O, A, H, W, image_id, palette, P, out: as csg_draw_boxes_u8, with its layouts, limits and alignment.
 * text: uint8, every label's bytes back to back; text_off: int32, B*O + 1 ascending offsets into it, text_off[0] == 0, on a
 * 4-byte boundary: row (b, o) owns the bytes [text_off[b*O+o], text_off[b*O+o+1]).  font: uint8 (95, 7): glyph g serves
 * byte 32 + g, row r (0 = top) is one byte whose bits 4..0 are the five columns from left to right.  All device memory.
 * Row o of sample b is skipped under csg_draw_boxes_u8's conditions, and when its label is empty.  For the others
 * (px0, py0, px1, py1) is that entry point's pixel rectangle, by the same fp32 statements, and with n label bytes
 *   the strip is [px0, px1] x [py0, min(py1, py0 + 8)]: nine lines, clipped to the box;
 *   tw = 6 n - 1, rw = px1 - px0 + 1, tx = px0 + max(0, (rw - tw) / 2) in integer division: the text is centred when it
 *   fits, and otherwise starts at the left side and is cut at px1;
 *   a strip pixel (x, y) is INK when r = y - py0 - 1 lies in [0, 6], c = x - tx lies in [0, tw), c % 6 < 5 and bit
 *   4 - c % 6 of font[g][r] is set, g being the glyph of the label's byte c / 6: the byte - 32 for a byte in [32, 126],
 *   otherwise the glyph of '?'.
 * Among the rows whose strip holds a pixel the HIGHEST o decides: an ink pixel becomes (0, 0, 0), another strip pixel
 * (img + palette[o % P] + 1) >> 1 per channel (the reference's alpha 0.5 in integers, from the INPUT byte, not from another
 * row's result); a pixel in no strip keeps its byte.  One launch, capturable, no atomics, nothing is read back; each lane
 * decides its own pixels, so the bytes are the same on every run.
 * LIMITS: those of csg_draw_boxes_u8; no null pointer (an empty text still needs an address); text_off[B*O] < 2^31.  */
int csg_draw_labels_u8(const uint8_t* img, const float* boxes, const int64_t* objs, int64_t B, int64_t O, int64_t A,
                       int64_t H, int64_t W, int64_t image_id, const uint8_t* palette, int64_t P, const uint8_t* text,
                       const int32_t* text_off, const uint8_t* font, uint8_t* out, void* stream);

/* ---- scene-graph pictures: segments, arrowheads and labelled nodes on a blank canvas (csrc/overlay.hip) --------
 * The picture of the graph itself that scripts/run_model.py writes beside each generated one (img_%06d_sg.png, there by
 * GraphViz through sg2im/vis.py:draw_scene_graph): here the caller lays the graph out (canonicalsg2im_amd/sgdraw.py) and
 * this entry point paints B canvases, out (B,3,H,W) uint8 planar, from per-picture lists of primitives.  There is no input
 * picture: every byte of out is written.  All geometry is integer and exact; the kernel uses no floating point.
 *   prims     int32 (n_prims, 8), 16-byte aligned: one record per primitive, see below;
 *   prim_off  int32, B + 1 ascending offsets, prim_off[0] == 0: picture b owns the records [prim_off[b], prim_off[b+1]);
 *   text      uint8 (text_bytes): the nodes' labels; font: uint8 (95, 7) as for csg_draw_labels_u8;
 *   background, and every colour of a record: r | g << 8 | b << 16.                         All device memory.
 * RECORD, words w0 .. w7:  w0 = kind | param << 4 | ink << 8,  w1 .. w6 geometry,  w7 = colour.
 *   kind 0, SEGMENT:  w1 .. w4 = ax, ay, bx, by; param = thickness t in 1 .. 8.  With d = B - A, v = p - A, L2 = d.d,
 *     dot = v.d, cross = vx dy - vy dx, the pixel p = (x, y) is covered when
 *       L2 == 0 or dot <= 0:  4 |p - A|^2 <= t^2;      dot >= L2:  4 |p - B|^2 <= t^2;      otherwise:  4 cross^2 <= t^2 L2.
 *   kind 1, TRIANGLE: w1 .. w6 = x0, y0, x1, y1, x2, y2.  With area2 = cross(V1 - V0, V2 - V0) and the edge functions
 *     e0 = cross(V1 - V0, p - V0), e1 = cross(V2 - V1, p - V1), e2 = cross(V0 - V2, p - V2): covered when area2 != 0 and
 *     (all e_i >= 0 or all e_i <= 0) - both windings, the border included; a degenerate triangle covers nothing.
 *   kind 2, NODE:     w1 .. w4 = x0, y0, x1, y1, the inclusive rectangle; w5 = the label's first byte in text, w6 = its
 *     bytes n; param = corner radius r in 0 .. 8; colour = fill, ink = the label's colour.  With re = min(r, (x1 - x0) / 2,
 *     (y1 - y0) / 2) in integer division, a pixel of the rectangle is covered unless it lies in a corner square and
 *     outside the corner circle (top left: x < x0 + re, y < y0 + re and (x0+re-x)^2 + (y0+re-y)^2 > re^2; the others
 *     mirrored).  A covered pixel is INK when, with tw = 6 n - 1, tx = x0 + max(0, (x1-x0+1 - tw) / 2) and
 *     ty = y0 + max(0, (y1-y0+1 - 7) / 2):  c = x - tx lies in [0, tw), l = y - ty in [0, 7), c % 6 < 5 and bit 4 - c % 6
 *     of font[g][l] is set, g being csg_draw_labels_u8's glyph of the label's byte c / 6 (bytes outside [32, 126]: '?').
 *     Text wider or taller than the node is cut at the node's border.
 * Among a picture's records that cover a pixel the one with the HIGHEST index decides: the pixel takes its ink colour
 * where it is label ink, else its colour; no blending.  A pixel no record covers is `background`.  Records may lie partly
 * or wholly outside the canvas.  One launch, capturable, no atomics, nothing read back; each lane decides its own pixels, so
 * the bytes are the same on every run.
 * LIMITS (CSG_E_BADSHAPE): 1 <= B <= 65535; H and W in [1, 2048]; W % 4 == 0; no null pointer (empty prims and text still
 * need an address); prims on a 16-byte boundary, prim_off and out on a 4-byte one.  The caller builds the records and
 * holds them to: coordinates in [-4096, 4096], at most 4096 records per picture, t and r as above, label ranges inside
 * text (ops.draw_graph_u8 refuses the rest with ValueError).  The coordinate bound is what keeps the rule inside int64:
 * |v| <= 6143 and |d| <= 8192 per axis give |cross| < 2^28, so 4 cross^2 < 2^58; cross^2 alone does not fit int32.
 * Offsets beyond n_prims and label bytes beyond text_bytes are not read (the record range is cut, the byte draws '?'). */
int csg_draw_graph_u8(const int32_t* prims, int64_t n_prims, const int32_t* prim_off, const uint8_t* text,
                      int64_t text_bytes, const uint8_t* font, int64_t B, int64_t H, int64_t W, uint32_t background,
                      uint8_t* out, void* stream);

/* ---- decoded pictures -> the trainer's image tensor (csrc/preprocess.hip) ------------------------------
 * The per-sample transform of the reference's loader (sg2im/data/packed_coco.py:269-272: T.Resize(image_size), T.ToTensor(),
 * T.Normalize(mean, std)) for a batch of DIFFERENTLY SIZED 8-bit RGB pictures, the exact inverse direction of
 * csg_deprocess_u8.
 *   src        uint8, device: B interleaved RGB pictures back to back, dense rows of 3 * w_i bytes at ANY byte alignment;
 *   desc       int64 (B,3), device: (byte offset in src, h_i, w_i) per picture;  desc_host: the same rows in HOST memory,
 *              read during the call — every refusal below is decided from it, before the first launch, without a
 *              device synchronisation.  A device row that disagrees with what was validated (a stale buffer under a
 *              replayed graph) is re-checked on the device and that picture is skipped rather than read out of bounds;
 *   out        fp32 (B,3,H,W), contiguous NCHW, 16-byte aligned;
 *   out_u8     nullable: the resized picture, uint8 (B,H,W,3), 4-byte aligned;
 *   sub3, div3 three floats each, HOST memory: mean and std of T.Normalize as fp32 (0 / 1: ToTensor alone).
 * Resize is Pillow's 8-bit bilinear `resize((W, H))` restated exactly: per axis fp64 coefficients (scale = in / out,
 * support = max(scale, 1), triangle weights normalised by their in-order sum, rounded to 22-bit fixed point), integer
 * accumulation, the horizontal pass first into a uint8 intermediate (`workspace`), then the vertical pass; a pass whose size
 * does not change is skipped.  The coefficients are computed on the device, in fp64, by the block that uses them.  Then
 * float(byte) / 255, - sub3[c], / div3[c]: three correctly rounded fp32 operations, no contraction.  out_u8 EQUALS Pillow's
 * bytes and out EQUALS torch's bits on the host (tests/test_gpu_preprocess.py).
 * Two launches, always (the horizontal one's blocks return at once for a picture with w_i == W), stream ordered and
 * capturable; no atomics, nothing read back.  A captured pair serves any later batch of the same B in the same buffers
 * whose heights do not exceed the captured maximum and whose workspace need does not exceed the captured size.
 * ALIGNMENT: out 16 bytes, out_u8 and workspace 4 bytes (CSG_E_BADSHAPE otherwise); src any.
 * LIMITS: 1 <= B <= CSG_PREPROCESS_MAX_BATCH; every side (h_i, w_i, H, W) in 1 .. CSG_PREPROCESS_MAX_SIDE (CSG_E_BADSHAPE);
 * h_i <= CSG_PREPROCESS_MAX_SCALE * H and w_i <= CSG_PREPROCESS_MAX_SCALE * W, i.e. a table of 2 * 64 + 1 = 129 taps per output (Pillow's width; at most 128 are ever used)
 * (CSG_E_UNSUPPORTED); offset_i >= 0 and offset_i + 3 h_i w_i <= src_bytes (CSG_E_BADSHAPE).
 * csg_preprocess_workspace = sum_i 3 * h_i * W bytes.                                                                     */
#define CSG_PREPROCESS_MAX_SCALE 64
#define CSG_PREPROCESS_MAX_SIDE 8192
#define CSG_PREPROCESS_MAX_BATCH 1024
int64_t csg_preprocess_workspace(const int64_t* desc_host, int64_t B, int64_t W);
int csg_preprocess(const uint8_t* src, int64_t src_bytes, const int64_t* desc, const int64_t* desc_host, int64_t B, int64_t H,
                   int64_t W, const float* sub3, const float* div3, float* out, uint8_t* out_u8, uint8_t* workspace,
                   int64_t workspace_bytes, void* stream);

/* The same transform for pictures of 3 OR 4 bytes per pixel, chosen per picture: desc and desc_host are int64 (B,4) rows
 * (byte offset in src, h_i, w_i, bytes per pixel).  With 4, rows are 4 * w_i bytes and a pixel is R, G, B and a fourth byte
 * that is ignored: what Pillow's RGBA -> RGB conversion drops, so a decoded RGBA picture (CLEVR's renders) needs no pass on
 * the host.  The pass that reads the picture itself (the horizontal one, or the vertical one when w_i == W) loads such a
 * pixel as one dword when offset_i is a multiple of 4, byte by byte otherwise.  Output, workspace layout (the horizontal
 * result is 3 bytes per pixel), launches, ranges, alignment and the device's re-check of its row are those of csg_preprocess,
 * with 3 h_i w_i replaced by (bytes per pixel) h_i w_i; in addition src must be 4-byte aligned and a bytes-per-pixel entry
 * other than 3 or 4 is CSG_E_BADSHAPE.  The kernels are the two instantiations of one template: a batch of 3-byte
 * pictures gives the bits csg_preprocess gives (tests/test_gpu_clevr.py).                                              */
int64_t csg_preprocess_px_workspace(const int64_t* desc_host, int64_t B, int64_t W);
int csg_preprocess_px(const uint8_t* src, int64_t src_bytes, const int64_t* desc, const int64_t* desc_host, int64_t B, int64_t H,
                      int64_t W, const float* sub3, const float* div3, float* out, uint8_t* out_u8, uint8_t* workspace,
                      int64_t workspace_bytes, void* stream);

/* ---- CLEVR scene geometry -> object boxes (csrc/clevr.hip) ---------------------------------------------
 * The reference's extract_bounding_boxes (sg2im/data/packed_clevr_dialog.py:21-77) for a padded batch, one lane per object.
 *   geom    fp64 (B,O,5), device: pixel_coords[0], pixel_coords[1], 3d_coords[0..2] of every object;
 *   objs    int64 (B,O,A), device: attribute 0 is the shape id, 1 cube, 2 sphere, 3 cylinder (:121);
 *   rot     fp64 (B,2), device: directions['right'][0..1] = (cos, sin) of the scene;
 *   counts  int64 (B,), device: objects of the scene; rows at or beyond it are padding;
 *   objs_host, counts_host: the same two in HOST memory, read during the call — the refusals are decided from them,
 *           before the launch, without a device synchronisation; a device row that disagrees (a stale buffer under a replayed
 *           graph) is written as a padding row;
 *   boxes   fp32 (B,O,4), 16-byte aligned: (x_min, y_min, x_max - x_min, y_max - y_min), -1 in padding rows.
 * The reference computes in Python floats and rounds once, when the lists become a FloatTensor; so does this: fp64 in the
 * reference's association order (the second rotation line reads the x1 the first has overwritten; 6.9 * z1 * (15 - y1) /
 * 2.0 left to right; (1.3 * 10) / (10 + y1); the cylinder's upper height first, the lower one derived from it; the
 * divisors 320 and 480 whatever the picture's size), no contraction, one rounding to fp32: boxes EQUAL the reference's bits
 * (tests/golden/clevr_boxes.npz).  One launch, stream ordered and capturable; nothing is read back.
 * LIMITS: 1 <= B <= CSG_CLEVR_MAX_BATCH, 1 <= O <= CSG_CLEVR_MAX_OBJECTS, 1 <= A <= 64, 0 <= counts <= O, every shape id
 * below its scene's count in 1 .. 3 (CSG_E_BADSHAPE otherwise); geom, rot, objs, counts 8-byte aligned.                   */
#define CSG_CLEVR_MAX_BATCH 65535
#define CSG_CLEVR_MAX_OBJECTS 1024
int csg_clevr_boxes(const double* geom, const int64_t* objs, int64_t A, const double* rot, const int64_t* counts,
                    const int64_t* objs_host, const int64_t* counts_host, int64_t B, int64_t O, float* boxes, void* stream);

/* ---- Visual Genome object rows -> object ids and boxes (csrc/vg.hip) ------------------------------------
 * The per-object loop of the reference's __getitem__ (sg2im/data/packed_vg.py:110-125) and the padding of vg_collate_fn
 * (:186-205) for a padded batch, one lane per (sample, object) row.
 *   rows    int32 (B,O,5), device: name id, x, y, w, h of every chosen object, the box in pixels as the split file has it;
 *   sizes   int64 (B,2), device: (HH, WW) of the DECODED picture of the sample (:81);
 *   counts  int64 (B,), device: chosen objects of the sample; rows at or beyond it are padding;
 *   rows_host, sizes_host, counts_host: the same three in HOST memory, read during the call — the refusals are decided from
 *           them, before the launch, without a device synchronisation; a device row that disagrees (a stale buffer under a
 *           replayed graph: a name out of range, a size below 1) is written as a padding row;
 *   objs    int64 (B,O): the name id, 0 in padding rows (the collate's zeros, :193-196);
 *   boxes   fp32 (B,O,4), 16-byte aligned, one 16-byte store per row:
 *               ((float)((double)x / WW), (float)((double)y / HH), (float)((double)w / WW), (float)((double)h / HH)),
 *           -1 in padding rows (:203-205).
 * The reference divides Python floats, `float(x) / WW`, and rounds once when the list becomes a FloatTensor (:118-120); so
 * does this: boxes EQUAL the reference's bits (tests/golden/vg_samples.npz).  Nothing clips a box to the picture: the
 * reference does not.  The __image__ row is not written here (collate.packed_batch appends it).  One launch, stream
 * ordered and capturable; nothing is read back.
 * LIMITS: 1 <= B <= CSG_VG_MAX_BATCH; 1 <= O <= CSG_VG_MAX_OBJECTS (csg_canon_general_* takes 256 rows with __image__);
 * 0 <= counts <= O; HH, WW >= 1; every name id below its sample's count in 1 .. num_object_names - 1 (0 is __image__)
 * (CSG_E_BADSHAPE otherwise); sizes, counts, objs 8-byte aligned, rows 4-byte aligned.                                */
#define CSG_VG_MAX_BATCH 1024
#define CSG_VG_MAX_OBJECTS 255
int csg_vg_rows(const int32_t* rows, const int64_t* sizes, const int64_t* counts, const int32_t* rows_host,
                const int64_t* sizes_host, const int64_t* counts_host, int64_t num_object_names, int64_t B, int64_t O,
                int64_t* objs, float* boxes, void* stream);

/* ---- validation metric: box IoU of a padded batch (csrc/metrics.hip) ---------------------------------
 * The reference's jaccard (sg2im/metrics.py:4-36) behind remove_dummies_and_padding (sg2im/utils.py:66-71), with the clamp
 * of scripts/train.py:196 and the sums check_model keeps (:211-217).
 * boxes_pred, boxes_gt (B,O,4) fp32 xywh, 16-byte aligned; objs (B,O,A) int64.  An object is COUNTED when any of its four
 * ground-truth values differs from -1 and objs[b,o,0] != image_id (not remove_dummy_objects: that mask tests != 0).
 * boxes_pred is clamped to [0,1] as xywh, then both boxes become corner points; inter, the two areas,
 * union = (area_pred + area_gt) - inter and iou = inter / union are single correctly rounded fp32 operations in the
 * reference's order (no contraction): iou EQUALS the reference's bits.  0 / 0 (both boxes of zero area) is NaN; it fails
 * both comparisons and makes the sums NaN, as in the reference.
 * iou (B,O) fp32, 0 where not counted; counted (B,O) uint8; per_sample (B,4) fp64 = {sum iou, #(iou > 0.5), #(iou > 0.3),
 * #counted}; totals[4] fp64 += the same four over the batch (a running buffer the caller zeroes once).  The sums are
 * ordered (fixed trees, no atomics): bit-reproducible.  Two launches (one block per sample; a one-wave fold), stream
 * ordered and capturable; nothing is read back.
 * LIMITS: 1 <= B <= 65535, 1 <= O <= 2^20, 1 <= A <= 64 (CSG_E_BADSHAPE otherwise, before the first launch).          */
int csg_box_iou(const float* boxes_pred, const float* boxes_gt, const int64_t* objs, int64_t B, int64_t O, int64_t A,
                int64_t image_id, float* iou, uint8_t* counted, double* per_sample, double* totals, void* stream);

/* ---- layout metric: relation agreement of a padded batch (csrc/metrics.hip) --------------------------
 * Does a layout obey the triplets it was made from?  The datasets' location rule (sg2im/data/base_dataset.py:42-81) asked
 * of the pair (s, o) of every triplet (s, p, o), on predicted boxes.  (Added after revision 122 without a new revision
 * number: callers detect it by its symbol.)
 * boxes (B,O,4) fp32 xywh, 16-byte aligned, clamped to [0,1] as xywh as csg_box_iou clamps boxes_pred (a NaN stays NaN);
 * xc = x0 + 0.5f * w and yc = y0 + 0.5f * h are one correctly rounded fp32 addition each.  centers (B,O,2) fp32, 8-byte
 * aligned, or NULL: the centre (cx, cy) of a row is its row of centers, else (xc, yc).  triplets (B,T,3) and triplet_type
 * (B,T) int64.  pred_ids (host, 8 int32, distinct, each in [0, P)): __padding__ __in_image__ __below__ __above__
 * __left of__ __right of__ __inside__ __surrounding__, as csg_canon_build takes them.
 * A row is TESTED when p is one of the six location ids (not __padding__, __in_image__ or any other id).  A tested row
 * AGREES when the rule yields p:  __surrounding__ iff sx0 < ox0 && sxc > oxc && sy0 < oy0 && syc > oyc;  __inside__ iff
 * the four mirrored comparisons hold;  otherwise __right of__ / __left of__ by scx > ocx / scx < ocx and __below__ /
 * __above__ by scy > ocy / scy < ocy (one of each axis can hold at once).  A pair with a NaN in a clamped box value or in
 * a centre is tested and does not agree.
 * tested, agrees (B,T) uint8; per_sample (B,4,2) int64 = {agreeing, tested} by triplet type 0..3; totals (4,P,2) int64 +=
 * the same by type and predicate (a running buffer the caller zeroes once).  Integer sums by fixed trees, no atomics:
 * bit-reproducible.  Two launches (one block per sample; one wave per (type, relation)), stream ordered and capturable;
 * nothing is read back.  workspace: csg_relation_agreement_workspace(B) bytes, 8-byte aligned.
 * triplets_host / triplet_type_host (host copies of the two, both or neither): with them every tested row is checked
 * before the first launch — s or o outside [0, O), or a type outside [0, 4), is CSG_E_BADSHAPE.  Without them the rows
 * are known on the device alone: such a row is never dereferenced, and is written as not tested.
 * LIMITS: 1 <= B <= 65535, 1 <= O <= 2^20, 1 <= T <= 2^20, 1 <= P <= 4096 (CSG_E_BADSHAPE otherwise, before the first
 * launch; a short workspace is CSG_E_WORKSPACE).                                                                   */
int64_t csg_relation_agreement_workspace(int64_t B);
int csg_relation_agreement(const float* boxes, const float* centers, const int64_t* triplets, const int64_t* triplet_type,
                           const int64_t* triplets_host, const int64_t* triplet_type_host, int64_t B, int64_t O, int64_t T,
                           int64_t P, const int32_t* pred_ids, uint8_t* tested, uint8_t* agrees, int64_t* per_sample,
                           int64_t* totals, void* workspace, int64_t workspace_bytes, void* stream);

/* ---- layout metric: consistency of two layouts of the same objects (csrc/metrics.hip) ----------------
 * The robustness run's metric: layout A from a graph, layout B from its rewritten graph.  (Added after revision 122 without
 * a new revision number, as the three entries below: callers detect them by their symbols.)
 * boxes_a, boxes_b (B,O,4) fp32 xywh, 16-byte aligned, BOTH clamped to [0,1] as xywh (a NaN stays NaN); counted (B,O) uint8,
 * the mask csg_box_iou writes.  Per counted object: iou_ab = csg_box_iou's jaccard of the two clamped boxes, the same
 * correctly rounded fp32 operations in the same order; shift = |axc - bxc| + |ayc - byc| with xc = x0 + 0.5f * w, every
 * step one fp32 operation; both (B,O) fp32, 0 where not counted.  Per ORDERED pair (i, j), i != j, of counted objects and
 * per location relation (slots below 0, above 1, left of 2, right of 3, inside 4, surrounding 5): the verdict of
 * csg_relation_agreement's rule with box centres on layout A and on layout B; a NaN in a pair makes all of that
 * layout's verdicts false.
 * per_sample_f (B,4) fp64 = {sum iou_ab, #(iou_ab > 0.5), sum shift, #counted}: thread o holds object o, a shuffle tree
 * (offsets 32 .. 1) per wave of 64, then waves 1, 2, 3 added to wave 0 in order.  per_sample_i (B,20) int64 = {in_a, in_b,
 * in_both} per slot, then same_pairs (the six verdicts identical in A and B) and pairs.  totals_f[4] fp64 and totals_i[20]
 * int64 += the samples in ascending sample order (running buffers the caller zeroes once).  No atomics: bit-reproducible.
 * Two launches (one block per sample; the fold), stream ordered and capturable; nothing is read back.
 * LIMITS: 1 <= B <= 65535, 1 <= O <= 256 (CSG_E_BADSHAPE otherwise, before the first launch).                         */
int csg_layout_consistency(const float* boxes_a, const float* boxes_b, const uint8_t* counted, int64_t B, int64_t O,
                           float* iou_ab, float* shift, double* per_sample_f, int64_t* per_sample_i, double* totals_f,
                           int64_t* totals_i, void* stream);

/* ---- graph rewriting for the robustness run (csrc/rewrite.hip; the hash and the row rules: csrc/csg_rewrite.h) ---------
 * csg_graph_rows_select: a sample's rows that are of type 0 (ORIGINAL) and carry one of the six location predicates, in
 * input order.  triplets (B,T,3), triplet_type (B,T) int64; pred_ids as csg_relation_agreement takes them.  rows (B,T,3)
 * int64 (not triplets): the selected rows, then [0, __padding__, 0]; counts (B,) int64: their number.  Such a row whose
 * subject or object lies outside [0, O) is dropped and the count is then NEGATIVE (-1 - the count), the convention of
 * csg_canon_general_build_dev.  One block per sample, an in-block prefix sum; one launch.
 * LIMITS: 1 <= B <= 65535, 0 <= T <= 2^20, 1 <= O <= 2^31, 1 <= P <= 4096.
 *
 * csg_graph_rewrite: out (B,R,3) = rows (B,R,3), the first counts[b] rows of each sample rewritten (a negative count:
 * none); out may be rows.  The row count never changes; duplicates may appear.  image_id (B,) int64 on the device.
 * h = the splitmix64-finaliser chain of csg_rewrite.h over (seed, image_id[b], a << 32 | b, slot); a row is selected when
 * (h >> 32) < floor(share * 2^32 + 0.5).
 * mode CSG_REWRITE_ONE_SIDED (0): the key is the row's forward form (a, b, slot_f) — a row of below, right of or
 * surrounding has subject and object swapped and its slot ^ 1.  A selected row becomes the forward form (direction 0), the
 * backward form (b, a, slot_f ^ 1) (1), or the one a coin of one more round names (2): both mirrored rows of a pair land
 * on the same form.  mode CSG_REWRITE_NOISE (1): the key is the row as given; a selected row's predicate becomes one of
 * the other five location predicates, uniformly, by ascending slot.  Integers only: the host restates every row exactly.
 * Refused before any launch (CSG_E_BADSHAPE): share outside [0, 1] or NaN, an unknown mode or direction, predicate ids
 * outside [0, P) or not distinct, a null operand, 1 <= B <= 65535, 0 <= R <= 2^20, 1 <= P <= 4096.  One launch.
 * Both entries are stream ordered and capturable, use no atomics and read nothing back.                              */
#define CSG_REWRITE_ONE_SIDED 0
#define CSG_REWRITE_NOISE 1
#define CSG_REWRITE_FORWARD 0
#define CSG_REWRITE_BACKWARD 1
#define CSG_REWRITE_RANDOM 2
int csg_graph_rows_select(const int64_t* triplets, const int64_t* triplet_type, int64_t B, int64_t T, int64_t O, int64_t P,
                          const int32_t* pred_ids, int64_t* rows, int64_t* counts, void* stream);
int csg_graph_rewrite(const int64_t* rows, const int64_t* counts, const int64_t* image_id, int64_t B, int64_t R, int64_t P,
                      const int32_t* pred_ids, int mode, int direction, double share, uint64_t seed, int64_t* out,
                      void* stream);

/* ---- K7 / pooling ------------------------------------------------------------------------------
 * nearest 2x upsample (generator.py:48,102-121) and its adjoint */
/* F.interpolate(x, size=(OH, OW), mode='nearest') of an NHWC map (B,IH,IW,C), C a multiple of 4 — the resize of the
 * segmentation map in SPADE.forward (spade/models/networks/normalization.py:98) when the caller passes a plain tensor
 * instead of the layout pyramid; the backward sums dy over the output pixels that read each input pixel, in order. */
int csg_nearest_resize_fwd(const float* x, int64_t B, int64_t IH, int64_t IW, int64_t C, int64_t OH, int64_t OW, float* y,
                           void* stream);
int csg_nearest_resize_bwd(const float* dy, int64_t B, int64_t IH, int64_t IW, int64_t C, int64_t OH, int64_t OW, float* dx,
                           void* stream);
int csg_upsample2x_fwd(const float* x, int64_t B, int64_t H, int64_t W, int64_t C, float* y, void* stream);
int csg_upsample2x_bwd(const float* dy, int64_t B, int64_t H, int64_t W, int64_t C, float* dx, void* stream);
/* F.avg_pool2d(3, stride 2, pad 1, count_include_pad=False) (discriminator.py:92-93) */
int csg_avgpool3s2_fwd(const float* x, int64_t B, int64_t H, int64_t W, int64_t C, float* y, void* stream);
int csg_avgpool3s2_bwd(const float* dy, int64_t B, int64_t H, int64_t W, int64_t C, float* dx, void* stream);
/* dx = add + avgpool_bwd(dy): the gradient of a map that feeds a consumer of its own (gradient `add`, laid out like dx; may BE
 * dx) and its pooled copy — MultiscaleDiscriminator's input (discriminator.py:120-131).  Replaces autograd's separate addition. */
int csg_avgpool3s2_bwd_add(const float* dy, int64_t B, int64_t H, int64_t W, int64_t C, const float* add, float* dx,
                           void* stream);

/* ---- object crops for the object discriminator (sg2im/bilinear.py:44-94) ---------------------------
 * out[n, y, x, c] = bilinear sample (grid_sample, align_corners=False, zeros padding) of image
 * img_idx[n] over box n ([x0,y0,w,h] in [0,1]); img is NHWC with img_cs floats per pixel, C used;
 * out is (N,HH,WW,out_cs) with channels >= C written as 0.  Backward: dimg is OVERWRITTEN — every image pixel gathers the
 * contributions of the crops that sampled it, in crop order (no atomics, bit-reproducible).
 * LIMITS of csg_crop_bwd: C <= 4 and HH, WW <= 64 (CSG_E_UNSUPPORTED otherwise; the reference crops 3-channel images at
 * --crop_size 32).  The forward and csg_crop_bwd_boxes have no such limit; the Python wrapper refuses a differentiable
 * crop outside them at FORWARD time. */
int csg_crop_fwd(const float* img, int64_t B, int64_t H, int64_t W, int64_t img_cs, int64_t C, const float* boxes,
                 const int64_t* img_idx, int64_t N, int64_t HH, int64_t WW, float* out, int64_t out_cs, void* stream);
int csg_crop_bwd(const float* dout, int64_t B, int64_t H, int64_t W, int64_t img_cs, int64_t C, const float* boxes,
                 const int64_t* img_idx, int64_t N, int64_t HH, int64_t WW, int64_t out_cs, float* dimg, void* stream);
/* Gradient w.r.t. the crop boxes (N,4) [x0,y0,w,h] — the sampling grid of crop_bbox is differentiable in them
 * (sg2im/bilinear.py:83-94); img is the forward's image, dboxes (N,4) is overwritten.  One block per crop, ordered sums. */
int csg_crop_bwd_boxes(const float* dout, const float* img, int64_t B, int64_t H, int64_t W, int64_t img_cs, int64_t C,
                       const float* boxes, const int64_t* img_idx, int64_t N, int64_t HH, int64_t WW, int64_t out_cs,
                       float* dboxes, void* stream);

/* ---- perceptual loss helpers (spade/models/networks/architecture.py:93-123, loss.py:102-117) --------
 * nn.MaxPool2d(kernel 2, stride 2) of torchvision's vgg19().features (floor mode; the backward
 * routes each gradient to the first maximum of its window, as ATen does, and needs the pool's
 * input x); nn.L1Loss() between two feature maps of n floats: out[0] = mean |a - b|, and
 * da = sign(a - b) * gout[0] / n.  The workspace holds per-block fp64 partial sums. */
int csg_maxpool2_fwd(const float* x, int64_t B, int64_t H, int64_t W, int64_t C, float* y, void* stream);
int csg_maxpool2_bwd(const float* dy, const float* x, int64_t B, int64_t H, int64_t W, int64_t C, float* dx,
                     void* stream);
/* nn.AvgPool2d(2, 2) of `build_cnn(pooling='avg')` (sg2im/layers.py:88-90): mean of each 2 x 2 window, floor mode */
int csg_avgpool2_fwd(const float* x, int64_t B, int64_t H, int64_t W, int64_t C, float* y, void* stream);
int csg_avgpool2_bwd(const float* dy, int64_t B, int64_t H, int64_t W, int64_t C, float* dx, void* stream);
int64_t csg_l1_mean_workspace(int64_t n);
int csg_l1_mean_fwd(const float* a, const float* b, int64_t n, float* out, void* workspace, int64_t workspace_bytes,
                    void* stream);
int csg_l1_mean_bwd(const float* a, const float* b, const float* gout, int64_t n, float* da, void* stream);

/* ---- GAN terms on the PatchGAN's prediction maps (spade/models/networks/loss.py:60-93, gan_mode hinge / w) in one launch:
 * out[0] = (1/n) sum_i -mean(term(x_i)) over up to four scales, term = x (kind 0: the generator's term), min(x - 1, 0)
 * (kind 1: discriminator on real), min(-x - 1, 0) (kind 2: discriminator on fake).  A map is (B, 1, H, W) with element strides
 * (sb, sh, sw); the backward writes d x_i into the contiguous (B, H, W) buffer dx.  fp64 sums in a fixed order. */
typedef struct csg_hinge_item {
  const float* x;
  float* dx;                    /* backward only */
  int64_t sb, sh, sw;
  int64_t B, H, W;
} csg_hinge_item;
int csg_hinge_mean_fwd(const csg_hinge_item* items, int32_t n, int32_t kind, float* out, void* stream);
int csg_hinge_mean_bwd(const csg_hinge_item* items, int32_t n, int32_t kind, const float* gout, void* stream);

/* ---- canonical scene-graph construction of the packed datasets -----------------------------------
 * Replaces, per batch, the per-sample numpy/python pipeline of the data loader:
 * BaseDataset.add_location_triplets -> add_dummy_triplets -> add_learnt_triplets (learned_converse=0)
 * (sg2im/data/base_dataset.py:35-151, scripts/graphs_utils.py:15-100; call order
 * sg2im/data/packed_clevr_dialog.py:205-209) and the triplet padding of the collate function
 * (packed_clevr_dialog.py:309-315).  Inputs are the padded batch tensors: objs0 (B,O) int64 ids of the
 * first attribute, boxes (B,O,4) xywh fp32, centers (B,O,2) fp32 (the dataset's obj_centers), n_objs (B,)
 * int64 number of objects of each sample INCLUDING its __image__ object (rows >= n are padding).
 * pred_ids[8] = ids of __padding__, __in_image__, __below__, __above__, __left of__, __right of__,
 * __inside__, __surrounding__.  At most 256 objects per sample.
 *   csg_canon_build: relations, transitive closure and reduction as bit matrices (kept in `workspace`,
 *     csg_canon_workspace(B) bytes) and counts[b] = {original triplets, transitive triplets}.
 *   csg_canon_emit: triplets (B,T,3) int64 sorted by (s,p,o) as np.unique(axis=0) does, then the
 *     transitive extras by (p,s,o); rows past a sample's count are [0, __padding__, 0];
 *     triplet_type (B,T) int64 is 0 / 1 (ORIGINAL_EDGE / TRANSITIVE_EDGE) and 0 in the padding.
 *     T is chosen by the caller: max_b(counts[b][0] + counts[b][1]) reproduces the collate. */
int64_t csg_canon_workspace(int64_t B);
int csg_canon_build(const int64_t* objs0, const float* boxes, const float* centers, const int64_t* n_objs,
                    int64_t B, int64_t O, const int32_t* pred_ids, int64_t image_id, int include_dummies,
                    int learned_transitivity, void* workspace, int64_t workspace_bytes, int64_t* counts,
                    void* stream);
int csg_canon_emit(const int64_t* objs0, const int64_t* n_objs, int64_t B, int64_t O, const int32_t* pred_ids,
                   int64_t image_id, int include_dummies, int learned_transitivity, const void* workspace,
                   const int64_t* counts, int64_t T, int64_t* triplets, int64_t* triplet_type, void* stream);
/* learned_converse = 1 (base_dataset.py:104-107; get_edge_converse_triplets, scripts/graphs_utils.py:126-152), between
 * csg_canon_build and csg_canon_emit: one uniform number per original triplet of the six location relations (the order of
 * the reference's loops: relations by ascending predicate id, triplets by (s, o); counts[b][0] minus the __in_image__
 * dummies of sample b) picks, through `cdf` (6 x 6 float64: per relation — in the order __below__ __above__ __left of__
 * __right of__ __inside__ __surrounding__ — the cumulative distribution numpy.random.choice forms from the softmax of the
 * five candidate weights, candidates by ascending predicate id, and a zero for "none"), whether a converse edge (o, r, s)
 * joins relation r.  `uniforms` is the host's random stream, `u_off[b]` the first number of sample b.  The workspace is
 * updated in place (current graph, transitive extras, offsets), `counts` rewritten, conv_counts (B, P, P + 1) float32 —
 * zero-initialised by the caller — receives the draw counts with column P = "none".                                    */
int csg_canon_converse(const int64_t* objs0, const int64_t* n_objs, int64_t B, int64_t O, const int32_t* pred_ids,
                       int64_t image_id, int include_dummies, int learned_transitivity, void* workspace,
                       const double* cdf, const double* uniforms, const int64_t* u_off, int64_t num_preds,
                       float* conv_counts, int64_t* counts, void* stream);

/* ---- canonical graphs with annotated relationships, any vocabulary -------------------------------------------------
 * The same pipeline for a sample's annotated (s, p, o) rows and every predicate of the vocabulary, in the order
 * sg2im/data/packed_vg.py:127-142 runs it (replacing, per batch, that loop and the triplet padding of vg_collate_fn,
 * packed_vg.py:207-212): the annotated rows (duplicates, self-relations and cycles allowed; never reduced), the location
 * relations of the geometry reduced per relation as csg_canon_build does (base_dataset.py:35-87), the __in_image__
 * dummies (:141-151), np.unique, then add_learnt_triplets (:89-139) over EVERY non-meta predicate by ascending id:
 * converse draws among all other non-meta predicates and "none" (scripts/graphs_utils.py:126-152), transitive extras of
 * each predicate's rows including the converse edges drawn into it (graphs_utils.py:15-27,96-100; cycles give (i, p, i)).
 * Output as csg_canon_emit: originals by (s, p, o), then the extras by (p, s, o), rows past a sample's count
 * [0, __padding__, 0] with type 0.
 *
 * roles (host, P int32): per predicate id, CSG_CANON_ROLE_PADDING, CSG_CANON_ROLE_IN_IMAGE, the location slot 0..5
 * (__below__ __above__ __left of__ __right of__ __inside__ __surrounding__) or CSG_CANON_ROLE_OTHER; each of the first
 * eight exactly once.  Ids may come in any order.
 * Call order: _build, [_converse], _close, then _emit with T = max_b(counts[b][0] + counts[b][1]).
 *   csg_canon_general_build: objs0 / boxes / centers as for csg_canon_build (device), or boxes = centers = NULL: no
 *     geometry, the location relations are the given rows alone (authored graphs); n_objs (host, B) objects per sample
 *     incl. __image__; rel (host, (B,R,3) int64) the annotated rows in local object indices, a sample's first
 *     rel_counts[b] rows (host, B), or with rel_counts NULL every row whose predicate is not __padding__.  Everything is
 *     checked before anything is enqueued; the rows are copied into the workspace on `stream`.  counts[b] = {number of
 *     draws of sample b (its original rows of non-meta predicates), 0}.
 *   csg_canon_general_converse (learned_converse = 1): cdf (P, K) float64, K = the number of non-meta predicates: row rel
 *     = the cumulative distribution numpy.random.choice searches for relation rel (candidates = the other non-meta
 *     predicates by ascending id, then "none"; rows of meta predicates unused); uniforms / u_off as for
 *     csg_canon_converse; conv_counts (B, P, P + 1) float32, zero-initialised by the caller, column P = "none".
 *   csg_canon_general_close: closure and counts[b] = {original triplets, transitive triplets}.
 *   csg_canon_general_emit: triplets (B,T,3) int64 and triplet_type (B,T) int64.
 * LIMITS: at most 256 objects per sample (O <= 256, CSG_E_UNSUPPORTED) and at most 256 predicates (P <= 256,
 * CSG_E_UNSUPPORTED); B * R < 2^31; an annotated object index outside [0, n_objs[b]), a predicate id outside [0, P), a
 * __padding__ row among a sample's counted rows, n_objs[b] outside [0, O] or a bad role table is CSG_E_BADSHAPE.
 * Workspace: csg_canon_general_workspace(B, P, R) bytes (about B * (P * 18 KB + 103 KB) + B * R * 4); the later
 * entries take the same workspace and size.                                                                                       */
#define CSG_CANON_ROLE_OTHER (-1)
#define CSG_CANON_ROLE_PADDING (-2)
#define CSG_CANON_ROLE_IN_IMAGE (-3)
int64_t csg_canon_general_workspace(int64_t B, int64_t P, int64_t R);
int csg_canon_general_build(const int64_t* objs0, const float* boxes, const float* centers, const int64_t* n_objs,
                            int64_t B, int64_t O, const int64_t* rel, const int64_t* rel_counts, int64_t R,
                            const int32_t* roles, int64_t P, int64_t image_id, int include_dummies, void* workspace,
                            int64_t workspace_bytes, int64_t* counts, void* stream);
int csg_canon_general_converse(int64_t B, const int32_t* roles, int64_t P, void* workspace, int64_t workspace_bytes,
                               const double* cdf, const double* uniforms, const int64_t* u_off, float* conv_counts,
                               void* stream);
int csg_canon_general_close(int64_t B, const int32_t* roles, int64_t P, int learned_transitivity, void* workspace,
                            int64_t workspace_bytes, int64_t* counts, void* stream);
int csg_canon_general_emit(int64_t B, const int32_t* roles, int64_t P, const void* workspace, int64_t workspace_bytes,
                           const int64_t* counts, int64_t T, int64_t* triplets, int64_t* triplet_type, void* stream);

/* csg_canon_general_build for annotated rows that are already ON THE DEVICE (the sampled pairs of csg_pair_relations).
 * Arguments as csg_canon_general_build, except: rel is a DEVICE pointer ((B,R,3) int64, 8-byte aligned); rel_counts (host, B)
 * is required: a sample's first rel_counts[b] rows are its rows and give the row offsets; boxes = centers = NULL
 * (CSG_E_UNSUPPORTED otherwise): the given rows are the whole graph, no location relation is derived.  The shapes, the
 * role table, n_objs and rel_counts are checked before anything is enqueued, with the messages of csg_canon_general_build
 * under this entry's name.  The rows cannot be: the kernel that packs them indexes nothing with a row whose object lies
 * outside [0, n_objs[b]), whose predicate lies outside [0, P) or is __padding__; it drops the row, and counts[b][0] of
 * that sample is then NEGATIVE (-1 - the count) after this entry and after csg_canon_general_close.  The caller reads
 * counts back for T anyway: on a negative one it must not call csg_canon_general_emit.  Then _converse / _close / _emit as
 * above, with the same workspace (csg_canon_general_workspace(B, P, R)). */
int csg_canon_general_build_dev(const int64_t* objs0, const float* boxes, const float* centers, const int64_t* n_objs,
                                int64_t B, int64_t O, const int64_t* rel, const int64_t* rel_counts, int64_t R,
                                const int32_t* roles, int64_t P, int64_t image_id, int include_dummies, void* workspace,
                                int64_t workspace_bytes, int64_t* counts, void* stream);

/* ---- canonical graphs of at most 64 rows per sample from annotated rows alone (reference sg2im/data/vg.py:136-149) ------
 * The unpacked Visual Genome dataset: the annotated rows and the __in_image__ dummies through add_learnt_triplets.  No
 * role table and no geometry: every predicate but pid_padding and pid_in_image is an ordinary non-meta predicate (a
 * vocabulary that has __left of__ is served the same way), and the output equals csg_canon_general_build(boxes = NULL) /
 * [_converse] / _close / _emit on the same rows, bit for bit.  A sample is one block and a predicate's 64x64 bit matrix one
 * 64-bit register per lane of a wave; csg_canon_small_build is ONE launch (scatter, draws, converse, closure, offsets),
 * csg_canon_small_emit a second one after the caller has read counts back for T = max_b(counts[b][0] + counts[b][1]).
 *   objs0 (B,O) int64 and n_objs (B,) int64 (rows per sample incl. __image__): device; n_objs_host: its host copy.
 *   rel (B,R,3) int64 in local indices: device, 8-byte aligned; rel_host: its host copy.  Rows of __padding__ are padding.
 *   cdf = NULL: no converse draws.  Otherwise cdf (P, K = P - 2) float64, uniforms, u_off (B,) int64 and conv_counts
 *   (B, P, P + 1) float32 (zero-initialised by the caller) as for csg_canon_general_converse, all on the device, and
 *   n_uniforms = the length of `uniforms`: the host counts a sample's draws itself, its distinct rows of non-meta
 *   predicates, so nothing is read back between the phases.
 *   counts (B,2) int64 (device) = {original triplets, transitive triplets}.
 * Checked on the host before anything is enqueued: P <= 256 and n_objs_host[b] <= 64 (CSG_E_UNSUPPORTED); n_objs_host[b] in
 * [0, O], every row of rel_host that is not padding with its predicate in [0, P) and both objects in [0, n_objs_host[b]),
 * two distinct meta ids in [0, P), the workspace size (CSG_E_BADSHAPE).  The kernel reads the DEVICE copies; it indexes
 * nothing with a row that fails those checks, nor `uniforms` past n_uniforms: counts[b][0] of such a sample is NEGATIVE
 * (-1 - the count), and the caller must not call csg_canon_small_emit.
 * No entry synchronises or copies: both launches can be captured.  Workspace: csg_canon_small_workspace(B, P) bytes
 * (B * P * 1544, rounded up to 256 per sample).                                                                       */
int64_t csg_canon_small_workspace(int64_t B, int64_t P);
int csg_canon_small_build(const int64_t* objs0, const int64_t* n_objs, const int64_t* n_objs_host, int64_t B, int64_t O,
                          const int64_t* rel, const int64_t* rel_host, int64_t R, int64_t P, int64_t pid_padding,
                          int64_t pid_in_image, int64_t image_id, int include_dummies, int learned_transitivity,
                          const double* cdf, const double* uniforms, const int64_t* u_off, int64_t n_uniforms,
                          float* conv_counts, void* workspace, int64_t workspace_bytes, int64_t* counts, void* stream);
int csg_canon_small_emit(int64_t B, int64_t P, int64_t pid_padding, const void* workspace, int64_t workspace_bytes,
                         const int64_t* counts, int64_t T, int64_t* triplets, int64_t* triplet_type, void* stream);

/* ---- the graph of the unpacked CLEVR dataset (reference sg2im/data/clevr_dialog.py:289-307, extract_triplets) -----------
 * The renderer's relation rows reduced per predicate to their minimal graph (scripts/graphs_utils.py:74-82,
 * reduce_transitive_edges with p_keep = keep, 0 or 1), then the __in_image__ dummies, then the collate's padding.  A sample
 * is one block, a predicate one wave, a row of its 64x64 bit matrix one lane.
 *   n_rows (B,) int64: rows per sample incl. its __image__ row, i.e. objects + 1: device; n_rows_host: its host copy.
 *   rel (B,R,3) int64 = [o2, pred, o1] as extract_triplets lists them (the relationships' key order, then o1 ascending,
 *   then the list's order, duplicates kept): device, 8-byte aligned; rel_host: its host copy.  Rows of __padding__ are
 *   padding and may stand anywhere.
 * Per predicate, in the order of the predicates' first rows: fewer than 3 listed rows are emitted as listed; otherwise
 * M = the rows as a matrix, H = hsu(path(M)) in the reference's in-place order (defined for cycles and self-relations
 * too), and H (keep = 0) or H | M (keep = 1) is emitted row-major.  Then [i, pid_in_image, n] for the n = n_rows - 1
 * objects, then [0, pid_padding, 0] up to T.  triplet_type is 0 (ORIGINAL_EDGE) everywhere.
 * csg_clevr_graph_count writes counts (B,) int64 (device) = triplets per sample, dummies included; the caller reads them
 * back for T = max_b counts[b] and calls csg_clevr_graph_emit with the same rows, which computes the same graphs again
 * and stores them: there is no workspace.
 * Checked on the host before anything is enqueued: P <= 16 and n_rows_host[b] <= 64 (CSG_E_UNSUPPORTED); n_rows_host[b] in
 * [1, O], every row of rel_host that is not padding with its predicate in [0, P) and both objects in [0, n), two distinct
 * meta ids in [0, P), keep in {0, 1} (CSG_E_BADSHAPE).  The kernels read the DEVICE copies and index nothing with a row
 * that fails those checks: counts[b] of such a sample is NEGATIVE (-1 - the count) and the caller must not emit.
 * No entry synchronises or copies: both launches can be captured.                                                     */
int csg_clevr_graph_count(const int64_t* n_rows, const int64_t* n_rows_host, int64_t B, int64_t O, const int64_t* rel,
                          const int64_t* rel_host, int64_t R, int64_t P, int64_t pid_padding, int64_t pid_in_image, int keep,
                          int64_t* counts, void* stream);
int csg_clevr_graph_emit(const int64_t* n_rows, int64_t B, int64_t O, const int64_t* rel, int64_t R, int64_t P,
                         int64_t pid_padding, int64_t pid_in_image, int keep, int64_t T, int64_t* triplets,
                         int64_t* triplet_type, void* stream);

/* ---- sampled-pair relations of the unpacked COCO dataset (reference sg2im/data/coco.py:372-421) ---------------------
 * Every object `cur` of a sample drew ONE other object and a coin on the host; this gives the pair's predicate, one thread
 * per (sample, object).  (s, o) = (cur, other[cur]), or (other[cur], cur) where flip[cur] != 0.  In fp32, in the reference's
 * order and without contraction: sx1 = sx0 + sw / 2 (the box centre: what the reference compares), likewise sy1, ox1, oy1;
 * __surrounding__ if sx0 < ox0 && sx1 > ox1 && sy0 < oy0 && sy1 > oy1, else __inside__ with every comparison reversed
 * (strict), else the quadrant of atan2(dy, dx), d = centers[s] - centers[o], decided WITHOUT atan2 by exact comparisons
 * that equal the reference's four double-precision inequalities for every fp32 pair: with ax = |dx|, ay = |dy|,
 * neg = signbit(dx): __left of__ if neg && ay <= ax; __right of__ if !neg && (ay < ax || (ay == ax && dy <= 0));
 * otherwise __above__ if dy < 0, else __below__.  use_converse != 0 (coco.py:404-421): __inside__ becomes __surrounding__,
 * __right of__ becomes __left of__ and __below__ becomes __above__, each with s and o swapped.
 * boxes (B,O,4) fp32 xywh, centers (B,O,2) fp32, counts (B,) int64 = rows per sample, other (B,O) int32, flip (B,O) uint8:
 * device; counts_host / other_host / flip_host: their host copies.  pred_ids (host, 8 int32): __padding__ __in_image__
 * __below__ __above__ __left of__ __right of__ __inside__ __surrounding__.  rows (B,O,3) int64 (device) receives (s, p, o);
 * a row at or beyond counts[b] is [0, __padding__, 0] — and so is one whose DEVICE `other` is not another counted row of
 * its sample (nothing is indexed with it).
 * Checked on the host before the launch (CSG_E_BADSHAPE): 0 <= counts_host[b] <= O; for every counted row
 * other_host[b][i] in [0, counts_host[b]) and != i, flip_host[b][i] in {0, 1}; distinct non-negative ids; alignment (boxes
 * 16, centers / counts / rows 8, other 4 bytes).  O <= 256 (CSG_E_UNSUPPORTED), as csg_canon_general_build requires. */
int csg_pair_relations(const float* boxes, const float* centers, const int64_t* counts, const int32_t* other,
                       const uint8_t* flip, const int64_t* counts_host, const int32_t* other_host, const uint8_t* flip_host,
                       int64_t B, int64_t O, const int32_t* pred_ids, int use_converse, int64_t* rows, void* stream);

/* ---- COCO segmentations -> M x M object masks and mask centroids (reference sg2im/data/packed_coco.py:305-351,
 * sg2im/data/coco.py:317-363; csrc/coco_masks.hip) -----------------------------------------------------------------
 * What the reference computes per object through pycocotools (frPyObjects / merge / decode) and OpenCV (cv2.resize,
 * INTER_NEAREST), restated from their public sources; the restatement is tests/mask_cases.py.  One block per (sample,
 * object) row; only the M source columns and M source rows the nearest-neighbour resize reads are evaluated.
 *   kind (B,O) uint8: 0 padding row, 1 a list of polygons, 2 run lengths.
 *   crop (B,O,4) int32 = x0, y0, x1, y1 of mask[y0:y1, x0:x1]: int(round(.)) of the annotation's box with ties to even,
 *     max(lo + 1, hi), clamped as a slice clamps — made on the host, from the annotation's own floats.
 *   sizes (B,2) int64 = (HH, WW) of the decoded pictures.   boxes (B,O,4) fp32 xywh over the picture's size.
 *   obj_poly (B,O,2) int32 = (first polygon, polygons) of a kind-1 row; poly_off (P+1,) int32: polygon p has the vertices
 *     poly_off[p] .. poly_off[p+1] of poly_xy (V,2) fp64 = (x, y) in pixels.  A polygon is rasterised as rleFrPoly does
 *     (scale 5, C truncation, one toggle per crossing of a pixel column's middle); an object's polygons are ORed.
 *   obj_runs (B,O,2) int32 = (first toggle, toggles) of a kind-2 row in toggles (T,) int32: the running sums of the
 *     column-major run lengths; pixel (x, y) is parity(#{toggles <= x * HH + y}).
 *   masks (B,O+1,M,M) int64, or NULL when only the centres are wanted: 0 / 1; rows of kind 0 are 0; row O of every sample,
 *     the __image__ row the collate appends, is all ones (packed_coco.py:330).
 *   centers (B,O,2) fp32: with count = sum of the mask, x0 + 0.5 w in fp32 for count == 0 (kind 0 included: the box centre),
 *     else x0 + ((fp32)(x0 + w) - x0) * sum_col / ((M - 1) * count) in fp64, rounded once; y likewise.
 * kind_host .. obj_runs_host: the host copies of the operands of those names.
 * Limits (CSG_E_UNSUPPORTED): M a power of two in 2 .. CSG_COCO_MASKS_MAX_M.  Checked on the host before the launch
 * (CSG_E_BADSHAPE): 1 <= B <= CSG_COCO_MASKS_MAX_BATCH, 1 <= O <= CSG_COCO_MASKS_MAX_OBJECTS; pictures of 1 ..
 * CSG_COCO_MASKS_MAX_SIDE on a side and fewer than 2^31 pixels; P, V <= CSG_COCO_MASKS_MAX_VERTICES; kind in {0, 1, 2}; for
 * every row that is not padding a non-empty crop inside the picture and its (first, count) inside [0, P] / [0, T];
 * poly_off non-decreasing inside [0, V]; every coordinate within +-CSG_COCO_MASKS_MAX_COORD; null operands (poly_xy may be
 * NULL with V == 0, toggles with T == 0); alignment (boxes 16, sizes / masks / centers / poly_xy 8, the int32 operands 4).
 * The kernel reads the DEVICE copies and indexes nothing with a row that fails those checks: it becomes a padding row.
 * No workspace, no synchronisation, no float atomics: capturable, and the same bytes on every run.                     */
#define CSG_COCO_MASKS_MAX_M 64
#define CSG_COCO_MASKS_MAX_BATCH 4096
#define CSG_COCO_MASKS_MAX_OBJECTS 256
#define CSG_COCO_MASKS_MAX_SIDE 16777216
#define CSG_COCO_MASKS_MAX_VERTICES 16777216
#define CSG_COCO_MASKS_MAX_COORD 1.0e6
int csg_coco_masks(const uint8_t* kind, const int32_t* crop, const int64_t* sizes, const float* boxes, const int32_t* obj_poly,
                   const int32_t* poly_off, const double* poly_xy, const int32_t* obj_runs, const int32_t* toggles,
                   const uint8_t* kind_host, const int32_t* crop_host, const int64_t* sizes_host, const int32_t* obj_poly_host,
                   const int32_t* poly_off_host, const double* poly_xy_host, const int32_t* obj_runs_host, int64_t B, int64_t O,
                   int64_t P, int64_t V, int64_t T, int64_t M, int64_t* masks, float* centers, void* stream);

/* ---- spectral normalisation of a conv weight (a13) ----------------------------------------------
 * torch.nn.utils.spectral_norm's forward pre-hook (reference call sites architecture.py:35-39,
 * normalization.py:27; SpectralNorm.compute_weight, n_power_iterations = 1, dim = 0):
 *   iterate != 0 (training): v <- normalize(W^T u); u <- normalize(W v), both buffers updated in place;
 *   sigma = u.(W v); w_eff = w / sigma.   normalize(x) = x / max(||x||, eps).
 * w is weight_orig viewed (Cout, K = Cin*KH*KW), K % 4 == 0.  u_used / v_used receive the vectors the
 * graph keeps for backward (PyTorch clones them for the same reason).
 * Backward: dw = (dweff - (sum dweff.w_eff) u v^T) / sigma; dweff is given with its element strides
 * along (Cout, Cin, KH, KW) — rows must be dense, e.g. contiguous or the [Cout][KH][KW][Cin] layout of
 * csg_conv_bwd_weight.  One workspace size serves both calls.
 * The calls take a list of weights — every spectrally normalised weight of a network pass in ONE launch per stage (a
 * generator forward calls the hook of architecture.py:35-39 on 18 convolutions, a PatchGAN pass on 3 per scale); one
 * weight is a list of one.  A weight's results do not depend on what shares its launch (bit for bit).  Per item:
 * `workspace` as csg_spectral_norm_workspace; cl_Cin = 0: W_eff in W's memory order; cl_Cin = Cin (a multiple of 4): W is
 * (Cout,Cin,KH,KW) row-major and W_eff is written in channels-last memory [Cout][KH][KW][Cin], the convolution kernels'
 * forward operand (no repack).                                                                                          */
int64_t csg_spectral_norm_workspace(int64_t Cout, int64_t K);
typedef struct csg_sn_fwd_item {
  const float* w;
  float* u;
  float* v;
  int64_t Cout, K;
  float* w_eff;
  int64_t cl_Cin;
  float* sigma;
  float* u_used;
  float* v_used;
  void* workspace;
  int64_t workspace_bytes;
} csg_sn_fwd_item;
int csg_spectral_norm_fwd_multi(const csg_sn_fwd_item* items, int32_t n, int32_t iterate, float eps, void* stream);
typedef struct csg_sn_bwd_item {
  const float* dweff;
  int64_t Cout, Cin, KH, KW, s0, s1, s2, s3;
  const float* w;
  const float* u_used;
  const float* v_used;
  const float* sigma;
  float* dw;
  void* workspace;
  int64_t workspace_bytes;
} csg_sn_bwd_item;
int csg_spectral_norm_bwd_multi(const csg_sn_bwd_item* items, int32_t n, void* stream);

/* ---- Inception-v3 forward and the statistics behind FID and the Inception score (csrc/inception.hip) ----------------
 * The network of evaluation/fid/inception.py:166-310 and torchvision's inception_v3 (evaluation/inception.py:16) runs its 94
 * convolutions through csg_conv_fwd; these are the passes around them.  All stream ordered and capturable, no atomics, every
 * sum in one fixed order.  Maps are NHWC fp32; channel counts, pixel strides and channel offsets are multiples of 4.
 *
 * csg_resize_bilinear: F.interpolate(mode='bilinear', align_corners=False), no antialiasing (fid/inception.py:146-150,
 * evaluation/inception.py:26), then a * x + b (fid/inception.py:153).  src: fp32 (B,IH,IW,src_cs) with src_cs 3 or 4 (src_u8 = 0)
 * or uint8 (B,IH,IW,3) (src_u8 = 1; a byte is first divided by 255 in fp32, fid_score.py:115).  out: fp32 (B,OH,OW,4), the
 * fourth channel 0; reverse = 1 writes the three channels in the opposite order (a BGR reader, fid_score.py:111).        */
int csg_resize_bilinear(const void* src, int32_t src_u8, int64_t B, int64_t IH, int64_t IW, int64_t src_cs, int64_t OH,
                        int64_t OW, float a, float b, int32_t reverse, float* out, void* stream);
/* 3x3 pool with (stride, pad) = (1, 1) or (2, 0).  kind 0: max, padding -inf (F.max_pool2d); 1: the sum divided by 9
 * (F.avg_pool2d, count_include_pad=True); 2: divided by the number of taps inside the picture (count_include_pad=False,
 * fid/inception.py:210).  The taps inside the picture are visited row by row, left to right, the averages start from 0 and
 * divide once: torch's host arithmetic, bit for bit.  x (B,H,W,x_cs), C channels read; y (B,OH,OW,y_cs), written at channels
 * [y_off, y_off + C) only.                                                                                            */
int csg_pool3(const float* x, int64_t B, int64_t H, int64_t W, int64_t C, int64_t x_cs, int32_t kind, int32_t stride,
              int32_t pad, float* y, int64_t y_cs, int64_t y_off, void* stream);
/* y (B,C) = mean over the P pixels of x (B,P,x_cs): adaptive_avg_pool2d(1) (fid_score.py:125-126).  B <= 65535. */
int csg_spatial_mean(const float* x, int64_t B, int64_t P, int64_t C, int64_t x_cs, float* y, void* stream);
/* y[p, y_off + c] = act(y[p, y_off + c] + bias[c]) in place, bias nullable: the epilogue of a convolution whose taps exceed
 * CSG_MAX_TAPS and which therefore is the SUM of two csg_conv_fwd launches over one weight (the second with accumulate = 1,
 * both without bias and activation) — InceptionA's 5x5 layers.                                                        */
int csg_bias_act(float* y, int64_t P, int64_t C, int64_t y_cs, int64_t y_off, const float* bias, int32_t act, float slope,
                 void* stream);
/* sum (D) += sum_n x[n], outer (D,D) += sum_n x[n] x[n]^T in fp64 from fp32 features x (n,D), rows in order; the caller zeroes
 * both before the first call.  D a multiple of 64.  A block owns a 64 x 64 tile of the upper triangle and mirrors it.
 * csg_feat_stats_finalize: mu = sum / N, sigma = (outer - N mu mu^T) / (N - 1) — np.mean(axis=0) and np.cov(rowvar=False)
 * (fid_score.py:213-214); N = 1 gives a NaN covariance, as numpy does.                                                */
int csg_feat_stats(const float* x, int64_t n, int64_t D, double* sum, double* outer, void* stream);
int csg_feat_stats_finalize(const double* sum, const double* outer, int64_t N, int64_t D, double* mu, double* sigma,
                            void* stream);
/* probs (N,K) fp64 = the fp32 row softmax of logits (N rows of ld floats): F.softmax of an fp32 model appended to a float64
 * array (evaluation/inception.py:28,33).                                                                               */
int csg_softmax_rows(const float* logits, int64_t N, int64_t K, int64_t ld, double* probs, void* stream);
/* compute_score (evaluation/inception.py:35-49) in fp64 over probs (N,K): split k is rows [k * (N / splits), (k + 1) * (N /
 * splits)); its score is exp(mean_i entropy(p_i, mean_i p_i)) with scipy.stats.entropy's renormalisation of both arguments.
 * out = [mean, population std, score of split 0, 1, ...] (2 + splits doubles).  1 <= splits <= N.                     */
int64_t csg_inception_score_workspace(int64_t N, int64_t K, int64_t splits);
int csg_inception_score(const double* probs, int64_t N, int64_t K, int64_t splits, double* workspace, int64_t workspace_bytes,
                        double* out, void* stream);

/* ---- KID and the object-level FID (SceneFID): the crop stage and the sums behind them (csrc/quality.hip) -------------
 * (Added after revision 122 without a new revision number: callers detect the entries by their symbols.)  As above: stream
 * ordered and capturable, no atomics, every sum in one fixed order, nothing read back.
 *
 * csg_crop_windows: boxes (N,4) fp32 [x, y, w, h] in units of the picture, 16-byte aligned -> windows (N,4) int32
 * [X0, Y0, X1, Y1), 16-byte aligned.  In fp32, one operation each: fx0 = x * W, fx1 = (x + w) * W;
 * X0 = clamp(floor(fx0), 0, W - 1), X1 = clamp(ceil(fx1), X0 + 1, W); likewise for y with H.  The conversion to int is
 * guarded: a value that is not >= 0 becomes 0 and a value above the side becomes the side, before the cast — every bit
 * pattern (NaN, +-inf) gives a window inside the picture with at least one pixel.  H and W in 1..16384.               */
int csg_crop_windows(const float* boxes, int64_t N, int64_t H, int64_t W, int32_t* windows, void* stream);
/* "Cut the window out, then csg_resize_bilinear it", one launch over all N crops: pictures uint8 (B,H,W,3), windows as
 * csg_crop_windows writes them, image_index (N) int32 -> out fp32 (N,OH,OW,4), the fourth channel 0.  Per crop the arithmetic
 * of csg_resize_bilinear on uint8 with the window as the whole picture, operation for operation: sy = (float)(Y1 - Y0) /
 * (float)OH, fy = max((oy + 0.5f) * sy - 0.5f, 0), the taps clamped to the window and offset by (Y0, X0), bytes / 255, the
 * same four products and three sums, a * v + b; reverse as there.  The kernel clamps the window to the picture (at least
 * one pixel) and image_index to [0, B) in integers before it forms an address: it reads inside `pictures` whatever the
 * two arrays hold.                                                                                                     */
int csg_crop_resize_bilinear(const uint8_t* pictures, int64_t B, int64_t H, int64_t W, const int32_t* windows,
                             const int32_t* image_index, int64_t N, int64_t OH, int64_t OW, float a, float b, int32_t reverse,
                             float* out, void* stream);
/* The three kernel sums of KID (Binkowski et al. 2018) for S subsets at once, no Gram matrix in memory.  fx (nx,D), fy (ny,D)
 * fp32, D a multiple of 64 (at most 8192); ix, iy (S,m) int32 row indices into them (clamped to the table before use).  With
 * k(u,v) = (gamma u.v + coef0)^degree, degree in {1,2,3}, over the subset's rows:
 *   out[s,0] = sum_{i != j} k(x_i,x_j)   out[s,1] = sum_{i != j} k(y_i,y_j)   out[s,2] = sum_{i,j} k(x_i,y_j)    (S,3) fp64.
 * A block owns a 64 x 64 tile of one matrix of one subset (xx and yy: the upper triangle, off-diagonal tiles doubled,
 * i = j skipped), a thread 4 x 4 dot products in fp64 registers, columns in order; a tile's 256 partial sums are added by
 * a fixed tree into the workspace, a second launch adds a matrix's tiles in index order.  Rows past m in the last tile
 * are masked, never read.  LIMITS: 2 <= m <= 65536 (CSG_E_BADSHAPE otherwise), 1 <= S <= 65535;
 * csg_kid_sums_workspace_bytes(S, m) bytes of workspace (-1 outside the limits), 8-byte aligned.                       */
int64_t csg_kid_sums_workspace_bytes(int64_t S, int64_t m);
int csg_kid_sums(const float* fx, int64_t nx, const float* fy, int64_t ny, int64_t D, const int32_t* ix, const int32_t* iy,
                 int64_t S, int64_t m, double gamma, double coef0, int32_t degree, void* workspace, int64_t workspace_bytes,
                 double* out, void* stream);
/* sums (C,D) fp64 += the rows of x (n,D) fp32 whose class_ids (n) int32 entry is the class, rows in order; counts (C) int64 +=
 * their number (running buffers the caller zeroes once).  One block per (class, 64-column slab); an id outside [0, C) is
 * skipped.  D a multiple of 64, at most 8192; C <= 65535.                                                             */
int csg_feat_class_sums(const float* x, const int32_t* class_ids, int64_t n, int64_t D, int64_t C, double* sums, int64_t* counts,
                        void* stream);

/* ---- k-nearest-neighbour manifolds: precision / recall, density / coverage (csrc/manifold.hip) -----------------------
 * (Added after revision 122 without a new revision number: callers detect the entries by their symbols.)  As above: stream
 * ordered and capturable, no atomics, nothing read back, the same bits on every run.  No n x m array exists in memory.
 *
 * THE DISTANCE, the only one both entries use: d2(u, v) = sum_c t_c * t_c with t_c = (double)u_c - (double)v_c, the columns
 * in ascending order, accumulated in fp64 with ONE FUSED multiply-add per column, acc = fma(t_c, t_c, acc).  It is the
 * difference form, not |u|^2 + |v|^2 - 2 u.v: identical rows are at exactly 0, d2(u, v) and d2(v, u) are the same bits, and
 * integer-valued features give the exact integer.  A NaN distance ranks as +inf; a NaN or +inf distance is "<=" nothing.
 *
 * csg_knn_radii: f (n,D) fp32, 16-byte aligned -> r2 (n) fp64: r2[i] = the k-th smallest of { d2(f_i, f_j) : j != i }.
 * Self is excluded by index, not by value: a duplicate row at another index counts, with distance 0; equal values count as
 * often as they occur.  With fewer than k finite distances r2[i] = +inf.  A block owns a 64 x 64 tile at a time (4 x 4 fp64
 * accumulators per thread), each row keeps its k smallest so far, one lane per row inserts a tile's candidates; when the
 * column tiles are cut into chunks, a second launch merges the chunks' k-lists in chunk order.
 * LIMITS (CSG_E_BADSHAPE otherwise): 1 <= k <= 16, k <= n - 1, n <= 2^20, D a multiple of 64, at most 8192.
 * csg_knn_radii_workspace_bytes(n, k) = chunks n k 8 bytes (-1 outside the limits), 8-byte aligned.
 *
 * csg_ball_counts: queries q (m,D), centres f (n,D), r2 (n) fp64 -> inside (m) int32, holds (n) int32:
 *   inside[j] = #{ i : d2(q_j, f_i) <= r2[i] }     holds[i] = #{ j : d2(q_j, f_i) <= r2[i] }
 * with "<=": a query on the sphere is inside.  A pair whose distance is NaN or +inf, or whose radius is NaN, is not counted
 * (so a centre with r2 = +inf holds every query at a finite distance and no other).  Both vectors come out of ONE pass over
 * the m x n pairs: the query tiles are cut into min(64, ceil(m / 64)) row groups and the centres into
 * csg_manifold_column_chunks(min(m, 4096), n) chunks, a block owns a (group, chunk) pair and is the only writer of its
 * partial counts; a second launch adds the groups and the chunks in index order.  Rows past m or n are masked, never read.
 * LIMITS: 1 <= m, n <= 2^20, D as above.  csg_ball_counts_workspace_bytes(m, n) = (m chunks + n groups) 4 bytes (-1
 * outside the limits), 4-byte aligned.
 *
 * csg_manifold_column_chunks(rows, cols), host only, no device needed: THE SPLIT RULE.  With ceil(rows / 64) blocks side by
 * side, the ceil(cols / 64) column tiles are cut into min(64, ceil(tiles / 2), ceil(8192 / blocks)) chunks, chunk c =
 * tiles [c tiles / chunks, (c + 1) tiles / chunks).  -1 unless 1 <= rows, cols <= 2^20.  csg_knn_radii uses (n, n).      */
int64_t csg_manifold_column_chunks(int64_t rows, int64_t cols);
int64_t csg_knn_radii_workspace_bytes(int64_t n, int64_t k);
int csg_knn_radii(const float* f, int64_t n, int64_t D, int64_t k, void* workspace, int64_t workspace_bytes, double* r2,
                  void* stream);
int64_t csg_ball_counts_workspace_bytes(int64_t m, int64_t n);
int csg_ball_counts(const float* q, int64_t m, const float* f, int64_t n, int64_t D, const double* r2, void* workspace,
                    int64_t workspace_bytes, int32_t* inside, int32_t* holds, void* stream);

/* ---- EMA of the weights: update, swap and fill of a flat fp32 shadow, one launch per call (csrc/ema.hip) --------------
 * (Added after revision 122 without a new revision number, as the entries above: callers detect them by their symbols.)
 * Stream ordered and capturable; no atomics, no host synchronisation, nothing read back; the same bits on every run.
 *
 * The work is an ITEM TABLE: item i pairs `numel` floats at `src` (a parameter or a floating buffer of the model) with
 * `numel` floats at `dst` (its slot in the shadow).  The shadow is ONE flat fp32 allocation; every slot starts at a
 * multiple of 4 floats, so src and dst are both 16-byte aligned (anything else is refused: there is no slow path), and
 * both are dense runs of numel floats.  numel = 0 is a legal item.
 *
 * WHERE THE TABLE LIVES: IN DEVICE MEMORY, built once when the shadow is made, because the storage of a model's tensors
 * stays where it is.  The multi-tensor entries above whose items change per call carry them in the kernel's arguments
 * and need one launch per 24-32 items; here one call is ONE launch for any number of items (at most CSG_EMA_MAX_ITEMS).
 * The host fills src / dst / numel / kind of a host copy, the planning entry below checks it and fills chunk0 (host only,
 * no device needed; returns the total number of chunks, or a negative code), the caller uploads the array (8-byte
 * aligned) and keeps it, and the tensors it names, alive while calls are in flight.
 *
 * WORK SPLIT: an item is cut into ceil(numel / CSG_EMA_CHUNK) chunks of CSG_EMA_CHUNK floats; a chunk never spans two
 * items; chunk0 is the number of chunks of the items before it.  A block takes a chunk at a time, finds its item by
 * bisection over chunk0, and moves 16 bytes per lane and stream; an item's last numel % 4 floats go one by one.
 *
 * MODES
 *   CSG_EMA_UPDATE  kind CSG_EMA_AVERAGE (parameters):  e' = fmaf(d, e, omd * p)  in fp32 — the product omd * p rounded,
 *                   then ONE fused multiply-add; this operation sequence is the contract (the tests' bound, two roundings,
 *                   is derived from it).  d = (float)D and omd = (float)(1.0 - (double)D) are made on the host, both in
 *                   [0, 1].  omd == 0 (D = 1) leaves AVERAGE items untouched, bit for bit.  D = 0 follows the formula,
 *                   fmaf(0, e, 1 * p): e = inf gives NaN.
 *                   kind CSG_EMA_COPY (running statistics, spectral-norm u / v):  e' = p, bit for bit.
 *   CSG_EMA_SWAP    p and e exchanged for every item, bit for bit (NaN payloads, signed zeros); twice is the identity.
 *   CSG_EMA_FILL    e = p for every kind (initialisation), bit for bit.  d and omd are ignored by SWAP and FILL.
 * Floats of the shadow outside the slots (the padding up to the next multiple of 4, anything behind the last slot) are
 * never read or written.                                                                                              */
#define CSG_EMA_AVERAGE 0
#define CSG_EMA_COPY 1
#define CSG_EMA_UPDATE 0
#define CSG_EMA_SWAP 1
#define CSG_EMA_FILL 2
#define CSG_EMA_CHUNK 4096
#define CSG_EMA_MAX_ITEMS 65536
typedef struct csg_ema_item {
  float* src;      /* the live tensor (written by SWAP only) */
  float* dst;      /* its slot in the shadow */
  int64_t numel;
  int64_t chunk0;  /* filled by the planning entry */
  int32_t kind;    /* CSG_EMA_AVERAGE | CSG_EMA_COPY */
  int32_t reserved;
} csg_ema_item;
int64_t csg_ema_table_plan(csg_ema_item* host_items, int64_t n);
int csg_ema_apply(const csg_ema_item* items, int64_t n, int64_t chunks, int32_t mode, float d, float omd, void* stream);

/* ---- DiffAugment of the discriminators' inputs: colour, translation, cutout; forward and adjoint (csrc/augment.hip) ---
 * (Added after revision 122 without a new revision number, as the entries above: callers detect them by their symbols.)
 * Stream ordered and capturable; no atomics, no host synchronisation, nothing read back; the same bits on every run.
 *
 * in / out: N samples of (H, H, Ct) floats, NHWC, dense, Ct a multiple of 4 (16-byte pixel rows), 16-byte aligned, not the
 * same buffer.  Colour channels are [c0, c0 + 3); c0 need not be a multiple of 4.  policy is a sum of CSG_AUG_COLOR,
 * CSG_AUG_TRANSLATION and CSG_AUG_CUTOUT; a policy that is off is skipped (policy 0 copies).  The transform, its order
 * (colour, translation, cutout), the zero fill and the exact fp32 operation sequence of the colour map: csrc/augment.hip.
 *
 * THE TABLE: one row of eight 32-bit words per sample, in device memory, 16-byte aligned: the fp32 bits of b, s, c, then
 * tx, ty, y0, x0, size as int32 (out[y, x] = in[y - ty, x - tx]; rows [y0, y0 + size) and columns [x0, x0 + size) are cut).
 * The transform entries read their parameters ONLY from it — nothing that varies per step is a kernel argument — and take
 * any values: every index is checked against the map.  The table entry fills `rows` rows from the counter-based hash of
 * csrc/csg_augment.h over (seed, iteration, pass, rank << 32 | row) with the ranges of the DiffAugment paper for maps of
 * H x H; its _host twin writes the same words to host memory (no device needed).
 *
 * The backward entry is the adjoint: `in` is the gradient at the transform's output, `out` the gradient at its input.
 * workspace: needed with CSG_AUG_COLOR only (8-byte aligned, the size the workspace entry returns): the per-sample sums
 * are a fixed fp64 tree over chunks of CSG_AUG_CHUNK pixels, so the bits do not depend on the grid.
 * Refused with a message (CSG_E_BADSHAPE): c0 + 3 > Ct, Ct % 4 != 0, H < 2 or H > CSG_AUG_MAX_H, table_rows < N,
 * N H H Ct >= 2^31, misaligned or null pointers, in == out, a workspace too small.                                      */
#define CSG_AUG_COLOR 1
#define CSG_AUG_TRANSLATION 2
#define CSG_AUG_CUTOUT 4
#define CSG_AUG_CHUNK 256
#define CSG_AUG_MAX_H 16384
int csg_augment_table(uint64_t seed, int64_t iteration, int64_t pass, int64_t rank, int64_t rows, int64_t H, uint32_t* table,
                      void* stream);
int csg_augment_table_host(uint64_t seed, int64_t iteration, int64_t pass, int64_t rank, int64_t rows, int64_t H,
                           uint32_t* table);
int64_t csg_augment_workspace_bytes(int64_t N, int64_t H);
int csg_augment_fwd(const float* in, float* out, const uint32_t* table, int64_t table_rows, int64_t N, int64_t H, int64_t Ct,
                    int64_t c0, int32_t policy, void* workspace, int64_t workspace_bytes, void* stream);
int csg_augment_bwd(const float* in, float* out, const uint32_t* table, int64_t table_rows, int64_t N, int64_t H, int64_t Ct,
                    int64_t c0, int32_t policy, void* workspace, int64_t workspace_bytes, void* stream);

/* ---- Adaptive strength of the augmentation (StyleGAN2-ADA, Karras et al., NeurIPS 2020): a per-sample gate, the
 * discriminator's overfitting figure and the controller of p, all on the device (csrc/augment.hip, csrc/csg_augment.h) ---
 * (Added after revision 122 without a new revision number: callers detect the entries by their symbols.)
 *
 * THE CONTROLLER RECORD: eight int64 words in device memory, 8-byte aligned, at an address that never changes:
 *     [p24, S, C, updates, S_last, C_last, 0, 0]
 * p = p24 * 2^-24 with p24 in [0, 2^24]; S = the sum of sign(x) and C = the number of elements x of the real pass's
 * prediction maps since the last update (sign: +1 for x > 0, -1 for x < 0, 0 for both zeros and NaN), so r_t = S / C.
 *
 * THE GATE: gate[n] is the mask (CSG_AUG_COLOR | _TRANSLATION | _CUTOUT) of the policies that are on for sample n: policy j is
 * on iff the 24-bit draw 8 + j of the sample's key is below p24.  The gate entry reads p24 from ctrl[0] ON THE DEVICE (a value
 * outside [0, 2^24] is clamped); its _host twin takes p24 as an argument.  The _gated transform entries are the ungated ones
 * plus `gate` (N int32, 4-byte aligned): sample n runs policy & gate[n]; a policy that is off for a sample is skipped for it
 * (colour off: the colour channels are bit copies; everything off: the sample is a bit copy, forward and backward).  The
 * ungated entries compute what they always did.
 *
 * csg_ada_accumulate adds to ctrl[1] and ctrl[2] over every element of 1..4 maps in the item form of csg_hinge_mean_fwd
 * (`dx` unused); the sums are integers (64-bit integer atomics, one pair per block): the same words whatever the grid.
 * csg_ada_update (one thread) applies   d = S 2^24 - T24 C;  p24 <- clamp(p24 + sgn(d) step24, 0, 2^24)   (C = 0 or d = 0:
 * unchanged), then S_last = S, C_last = C, S = C = 0, updates += 1; its _host twin does the same on host memory.
 * Refused with a message (CSG_E_BADSHAPE) before any launch: null or misaligned pointers, T24 outside [0, 2^24],
 * step24 < 1, and in the host entries p24 outside [0, 2^24] and C >= 2^38 (S 2^24 would leave int64; the device entry
 * leaves p24 alone there).                                                                                              */
int csg_augment_gate(uint64_t seed, int64_t iteration, int64_t pass, int64_t rank, int64_t rows, const int64_t* ctrl,
                     int32_t* gate, void* stream);
int csg_augment_gate_host(uint64_t seed, int64_t iteration, int64_t pass, int64_t rank, int64_t rows, int64_t p24, int32_t* gate);
int csg_augment_fwd_gated(const float* in, float* out, const uint32_t* table, int64_t table_rows, int64_t N, int64_t H,
                          int64_t Ct, int64_t c0, int32_t policy, void* workspace, int64_t workspace_bytes, const int32_t* gate,
                          void* stream);
int csg_augment_bwd_gated(const float* in, float* out, const uint32_t* table, int64_t table_rows, int64_t N, int64_t H,
                          int64_t Ct, int64_t c0, int32_t policy, void* workspace, int64_t workspace_bytes, const int32_t* gate,
                          void* stream);
int csg_ada_accumulate(const csg_hinge_item* items, int32_t n_items, int64_t* ctrl, void* stream);
int csg_ada_update(int64_t* ctrl, int64_t T24, int64_t step24, void* stream);
int csg_ada_update_host(int64_t* ctrl, int64_t T24, int64_t step24);

/* ---- The ADA augmentation pipeline: pixel blitting, general geometry and linear colour transforms as ONE per-sample
 * affine resampling with a 3 x 4 colour matrix, forward and exact adjoint (csrc/ada_pipeline.hip, csrc/csg_ada_pipeline.h) ---
 * (Added after revision 122 without a new revision number: callers detect the entries by their symbols.)
 * Stream ordered and capturable; no atomics, no host synchronisation, nothing read back; the same bits on every run.
 *
 * THE TABLE: one row of CSG_ADA_ROW_WORDS = 32 words of 32 bits per sample, in device memory, 16-byte aligned (the layout, the
 * draws, the fp64 composition and the polynomials: csrc/csg_ada_pipeline.h): the inverse map M (6 fp32), the forward map G
 * (6 fp32), the adjoint's search margin, a flag word, the integer map's offsets, the colour matrix (12 fp32) and the integer
 * map's signed permutation.  csg_ada_pipeline_table fills `rows` rows for H x H maps from the hash of (seed, iteration, pass,
 * rank << 32 | row) and from p24, which it reads from ctrl[0] ON THE DEVICE (clamped to [0, 2^24]); policy is a sum of
 * CSG_AUG_ADA_BLIT, CSG_AUG_ADA_GEOM and CSG_AUG_ADA_COLOR (the DiffAugment bits count for nothing here).  The _host twin
 * takes p24 as an argument and writes the same words to host memory (no device needed).
 *
 * in / out: N samples of (H, H, Ct) floats, NHWC, dense, Ct a multiple of 4, 16-byte aligned, not the same buffer.  Colour
 * channels are [c0, c0 + 3).  The transform entries read their parameters ONLY from the table and take any values: a
 * non-finite map or a coordinate of 2^23 or more gives zeros, every index is checked against the map, the adjoint's walk is
 * clamped to the map and to CSG_ADA_MAX_BOX pixels a side.  The operation sequences: csrc/ada_pipeline.hip.
 * Refused with a message (CSG_E_BADSHAPE) before any launch: c0 + 3 > Ct, Ct % 4 != 0, H < 2 or H > CSG_AUG_MAX_H,
 * table_rows < N, N H H Ct >= 2^31, misaligned or null pointers, in == out, policy outside the three bits, p24 outside
 * [0, 2^24] (host entry).                                                                                               */
#define CSG_AUG_ADA_BLIT 8
#define CSG_AUG_ADA_GEOM 16
#define CSG_AUG_ADA_COLOR 32
int csg_ada_pipeline_table(uint64_t seed, int64_t iteration, int64_t pass, int64_t rank, int64_t rows, int64_t H, int32_t policy,
                           const int64_t* ctrl, uint32_t* table, void* stream);
int csg_ada_pipeline_table_host(uint64_t seed, int64_t iteration, int64_t pass, int64_t rank, int64_t rows, int64_t H,
                                int32_t policy, int64_t p24, uint32_t* table);
int csg_ada_pipeline_fwd(const float* in, float* out, const uint32_t* table, int64_t table_rows, int64_t N, int64_t H, int64_t Ct,
                         int64_t c0, void* stream);
int csg_ada_pipeline_bwd(const float* in, float* out, const uint32_t* table, int64_t table_rows, int64_t N, int64_t H, int64_t Ct,
                         int64_t c0, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* CSG_HIP_H */
