"""Scene graphs -> uint8 pictures from a trained checkpoint (the reference's scripts/run_model.py,
scripts/generation_attspade.py and the samples of check_model: `model(objs, triplets, triplet_type, test_mode=True)`
followed by `deprocess_batch`, sg2im/data/utils.py:46-65).

`Sampler` owns a `MetaGeneratorModel` in eval mode (or adopts one: `model=`, evaluate.py) and nothing else (no discriminators, no optimisers).  The scene-graph
encoder runs as the module does; the generator is WALKED here on the inference forms of the kernels instead of through
`SPADEGenerator.forward` (whose eval-mode behaviour is untouched):

  * everything derived from the frozen weights is made once per `load` and held: W / sigma of the spectrally normalised
    weights (one multi-tensor pass without power iteration: u / v are not written), the gamma || beta joins, the kernels'
    weight layouts and Winograd operands, and (mean, invstd) of every SPADE norm's running statistics in one launch;
  * a SPADE modulation is one launch where F(4x4,3x3) serves the map (`ops.spade_infer`): neither gamma nor beta is written;
  * the picture leaves the device as uint8 (`ops.deprocess_u8`), bit-identical to the host's deprocess_batch;
  * the walk — layout pyramid through conv_img and the deprocess — is captured per (batch, padded objects, size, attributes,
    masks) key the second time the key is seen and replayed (`CSG_GRAPHS=0`: always eager); one stream, no branches.

`Sampler.generate_from_graphs` takes scene graphs a person wrote (authored.py: the reference's scripts/run_model.py form,
or a flat one) instead of a dataset's batch, and can draw the predicted boxes on the pictures (`ops.draw_boxes_u8`).
"""
import torch

from . import graphs as csg_graphs
from . import ops
from .sg2im.meta_models import MetaGeneratorModel
from .sg2im.utils import real_object_mask
from .spade.models.networks.normalization import InstanceNormAct, _joined
from .spectral_norm import HipSpectralNorm

NO_CPU = "canonicalsg2im_amd.sample needs a HIP device: there is no CPU path"


NO_EMA = ("checkpoint has no 'model_ema_state': it was written without an EMA of the weights — train with --ema_decay D "
          "(0 < D <= 1) to have one saved, or sample the raw weights (use_ema=False, --use_ema 0)")


def model_state_of(ckpt, use_ema=False):
    """`model_state` of a checkpoint dictionary written by `Trainer.save_checkpoint` or by the reference
    (scripts/train.py:488-520; its `gans_model_state` — DataParallel's `module.` keys — and the discriminator / optimiser
    entries are not needed here and not read).  A generator saved from inside a DataParallel wrapper loses its `module.`.
    `use_ema`: `model_ema_state` instead, the averaged weights a run with --ema_decay saves under the same keys (ema.py);
    a checkpoint without it is refused."""
    key = "model_ema_state" if use_ema else "model_state"
    if use_ema and key not in ckpt:
        raise KeyError(NO_EMA)
    if key not in ckpt:
        raise KeyError("checkpoint has no 'model_state' (keys: %s)" % sorted(ckpt))
    sd = ckpt[key]
    if sd and all(k.startswith("module.") for k in sd):
        sd = {k[len("module."):]: v for k, v in sd.items()}
    return sd


class _Replay:
    """One captured walk: static inputs, the graph, static outputs."""

    def __init__(self, B, O, A, M, device, obj_dtype):
        self.objs = torch.zeros((B, O, A), device=device, dtype=obj_dtype)
        self.boxes = torch.full((B, O, 4), -1.0, device=device, dtype=torch.float32)
        self.masks = torch.zeros((B, O, M, M), device=device, dtype=torch.float32) if M else None
        self.graph = self.img = self.u8 = None

    def load(self, objs, boxes, masks):
        O = objs.shape[1]
        if O < self.objs.shape[1]:                      # `__image__` rows: culled by the layout kernels (graphs.py)
            self.objs.zero_()
            self.boxes.fill_(-1.0)
            if self.masks is not None:
                self.masks.zero_()
        self.objs[:, :O].copy_(objs, non_blocking=True)
        self.boxes[:, :O].copy_(boxes, non_blocking=True)
        if self.masks is not None:
            self.masks[:, :O].copy_(masks, non_blocking=True)


class Sampler:
    def __init__(self, opt, device, checkpoint=None, model=None, use_ema=False):
        """`use_ema`: load the checkpoint's `model_ema_state` (the EMA of the weights, ema.py) instead of `model_state`.
        `model`: a MetaGeneratorModel to ADOPT instead of constructing one (the evaluator walks the trainer's own module:
        one copy of the weights).  Its mode is left alone here; `generate` puts it in eval mode and leaves it there.  Whoever
        trains an adopted model calls `invalidate()` before the next walk: a fused optimiser step and a replayed training
        step write parameters and running statistics without touching the `_version` counters `_signature` reads."""
        self.opt, self.device = opt, torch.device(device)
        if use_ema and checkpoint is None:
            raise ValueError("Sampler(use_ema=True) needs a checkpoint: the averaged weights are read from it")
        if model is None:
            model = MetaGeneratorModel(opt, self.device)
            model.eval()
        self.model = model
        self._prep = None                # everything derived from the frozen weights (see _prepare)
        self._replays, self._seen = {}, {}
        self.replays = self.eager_calls = 0
        if checkpoint is not None:
            self.load(checkpoint, use_ema=use_ema)

    # ------------------------------------------------------------------ weights
    def load(self, ckpt, use_ema=False):
        """Strict load of `model_state` (`use_ema`: of `model_ema_state`) from a checkpoint dictionary or a path to one;
        drops every preparation and graph."""
        if not isinstance(ckpt, dict):
            ckpt = torch.load(ckpt, map_location=self.device)
        self.model.load_state_dict(model_state_of(ckpt, use_ema), strict=True)
        self.model.eval()
        self.invalidate()

    def invalidate(self):
        self._prep = None
        self._replays, self._seen = {}, {}

    def _signature(self):
        """Changes whenever a tensor of the generator is replaced, moved (`module.to`) or written in place."""
        gen = self.model.layout_to_image_model.module
        return tuple((t.data_ptr(), t._version) for t in list(gen.parameters()) + list(gen.buffers()))

    def _prepare(self):
        """Once per loaded set of weights: W / sigma (no power iteration), gamma || beta joins, frozen layouts and Winograd
        operands, eval statistics.  Held here; `load` and anything that changes the generator's tensors drop it."""
        gen = self.model.layout_to_image_model.module
        if self._prep is not None and self._prep["sig"] == self._signature():
            return self._prep
        self._replays, self._seen = {}, {}
        spades, sn = [], []
        for m in gen.modules():
            if hasattr(m, "mlp_gamma") and hasattr(m, "mlp_beta"):
                if isinstance(m.param_free_norm, InstanceNormAct):
                    raise NotImplementedError("Sampler: SPADE over InstanceNorm has no running statistics to fold")
                spades.append(m)
            for hook in m._forward_pre_hooks.values():
                if isinstance(hook, HipSpectralNorm):
                    sn.append((m, hook))
        weff = {}
        if sn:
            eps = {float(h.eps) for _, h in sn}
            if len(eps) != 1:
                raise NotImplementedError("Sampler: spectral norms with different eps")
            outs = ops.spectral_weights([(getattr(m, h.name + "_orig"), getattr(m, h.name + "_u"), getattr(m, h.name + "_v"))
                                         for m, h in sn], False, eps.pop())
            weff = {m: w.detach() for (m, _), w in zip(sn, outs)}
        joins = {}
        for sp in spades:
            sp.joined_weight()
            _joined(sp, "_joined_b", sp.mlp_gamma.bias, sp.mlp_beta.bias)
            joins[sp] = (sp.__dict__["_joined_w"].detach(), sp.__dict__["_joined_b"].detach())
        packs = {}
        for m in gen.modules():
            if isinstance(m, torch.nn.Conv2d) and tuple(m.kernel_size) == (3, 3) and m is not gen.conv_img \
                    and not any(m is sp.mlp_gamma or m is sp.mlp_beta for sp in spades):
                w = weff.get(m)
                if w is None and hasattr(m, "weight_orig"):
                    continue
                packs[m] = ops.pack_frozen_forward(m.weight if w is None else w)
        for sp in spades:
            packs[sp] = ops.pack_frozen_forward(joins[sp][0])
        eps = {float(sp.param_free_norm.eps) for sp in spades}
        if len(eps) != 1:
            raise NotImplementedError("Sampler: SPADE norms with different eps")
        eps = eps.pop()
        stats = ops.norm_eval_stats([(sp.param_free_norm.running_mean, sp.param_free_norm.running_var) for sp in spades], eps)
        # the signature is taken AFTER the joins: they re-point the gamma / beta parameters into one allocation
        self._prep = {"weff": weff, "joins": joins, "packs": packs, "stats": dict(zip(spades, stats)), "eps": eps,
                      "scratch": {}, "sig": self._signature()}
        return self._prep

    # ------------------------------------------------------------------ the generator walk
    def _conv(self, m, x, residual=None):
        P = self._prep
        w = P["weff"].get(m, None)
        w = m.weight if w is None else w
        return ops.conv2d(x, w, m.bias, m.stride[0], m.padding[0], m.act, m.slope, residual, packs=P["packs"].get(m))

    def _mod(self, sp, x, seg, slope):
        P = self._prep
        w, b = P["joins"][sp]
        pn = sp.param_free_norm
        actv = self._conv(sp.mlp_shared[0], seg[int(x.size(2))])
        return (actv, w, b, pn.running_mean, pn.running_var, slope, P["packs"][sp])

    def _spade(self, x, seg, *pairs):
        P = self._prep
        key = (x.numel(), x.device)
        if key not in P["scratch"]:
            P["scratch"][key] = torch.empty(x.numel(), device=x.device, dtype=torch.float32)
        return ops.spade_infer(x, [self._mod(sp, x, seg, slope) for sp, slope in pairs], P["eps"],
                               stats=[P["stats"][sp] for sp, _ in pairs], scratch=P["scratch"][key])

    def _block(self, blk, x, seg):
        """SPADEResnetBlock.forward (architecture.py:50-68) in eval mode."""
        if blk.learned_shortcut:
            xs, h = self._spade(x, seg, (blk.norm_s, 1.0), (blk.norm_0, 0.2))
            x_s = self._conv(blk.conv_s, xs)
        else:
            x_s = x
            h, = self._spade(x, seg, (blk.norm_0, 0.2))
        dx = self._conv(blk.conv_0, h)
        h, = self._spade(dx, seg, (blk.norm_1, 0.2))
        return self._conv(blk.conv_1, h, residual=x_s)

    def _walk(self, objs, boxes, masks, uint8, rescale, deprocess="imagenet"):
        """SPADEGenerator.forward(test_mode=True) (generator.py:79-127): layout pyramid -> fc -> blocks -> conv_img [-> uint8]."""
        gen = self.model.layout_to_image_model.module
        if gen.sw != gen.sh:
            raise NotImplementedError("aspect_ratio != 1 is not on the hot path")
        H = gen.opt.image_size[0]
        levels = [gen.sw << k for k in range(H.bit_length()) if (gen.sw << k) <= H]
        valid = real_object_mask(objs, gen.opt.vocab)
        vecs = gen.attribute_embedding(objs)
        if masks is not None:                           # painter's compositing (layout.py:135-151)
            maps = ops.layout_paint(vecs, boxes, valid, masks, H, levels)
        else:
            maps = ops.layout_pyramid(vecs, boxes, valid, H, levels)
        seg = dict(zip(levels, maps))
        x = self._conv(gen.fc, seg[gen.sw])
        no_upsample = {"head_0"} | (set() if gen.opt.num_upsampling_layers in ('more', 'most') else {"G_middle_1"})
        for name in gen._block_names:
            if name not in no_upsample:
                x = ops.upsample2x(x)
            x = self._block(getattr(gen, name), x, seg)
        ci = gen.conv_img
        img = ops.conv2d(x, ci.weight, ci.bias, 1, ci.padding[0], ci.act, ci.slope, pre_slope=2e-1)
        return img, (ops.deprocess_u8(img, rescale, deprocess) if uint8 else None)

    def _generator(self, objs, boxes, masks, uint8, rescale, deprocess="imagenet"):
        B, O, A = objs.shape
        M = 0 if masks is None else int(masks.shape[-1])
        # the deprocess function's constants are baked into a captured walk: its name is part of the key
        key = (B, csg_graphs._pad_objects(O), int(self.opt.image_size[0]), A, M, bool(uint8), bool(rescale),
               str(deprocess) if uint8 else None)
        rp = self._replays.get(key)
        if rp is None:
            n = self._seen.get(key, 0)
            self._seen[key] = n + 1
            if not csg_graphs.ENABLED or n < csg_graphs.CAPTURE_AFTER or len(self._replays) >= csg_graphs.MAX_SETS:
                self.eager_calls += 1
                return self._walk(objs, boxes, masks, uint8, rescale, deprocess)
            rp = self._replays[key] = _Replay(B, key[1], A, M, objs.device, objs.dtype)
        rp.load(objs, boxes, masks)
        if rp.graph is None:
            g = torch.cuda.CUDAGraph()
            csg_graphs._quiesce_before_capture()
            with csg_graphs._Capture(g):
                rp.img, rp.u8 = self._walk(rp.objs, rp.boxes, rp.masks, uint8, rescale, deprocess)
            rp.graph = g
        rp.graph.replay()
        self.replays += 1
        # copies: the static outputs are overwritten by the next replay
        return rp.img.clone(), (None if rp.u8 is None else rp.u8.clone())

    # ------------------------------------------------------------------ public
    def generate(self, objs, triplets, triplet_type, boxes_gt=None, masks_gt=None, uint8=True, rescale=True,
                 deprocess="imagenet"):
        """(images, boxes_pred, masks_pred) of MetaGeneratorModel.forward(..., test_mode=True) (reference
        sg2im/meta_models.py:25-51): ground-truth boxes / masks win over the predictions where given; with masks the layout
        is painter's compositing.  images: uint8 (B,3,H,W) = deprocess_batch(imgs, rescale, <deprocess>) with `deprocess`
        "imagenet" or "decode_img" (ops.deprocess_u8), or with uint8=False the fp32 (B,3,H,W) image in channels-last memory.
        triplets=None with boxes_gt: the picture of that layout from the generator alone; the scene-graph encoder is not run
        and boxes_pred / masks_pred are None."""
        if self.device.type != "cuda" or not objs.is_cuda:
            raise RuntimeError(NO_CPU)
        if deprocess not in ops.DEPROCESS:
            raise ValueError("generate: deprocess must be one of %s, got %r" % (
                " or ".join(repr(k) for k in ops.DEPROCESS), deprocess))
        model = self.model
        with torch.no_grad():
            if model.training:
                model.eval()
            boxes_pred = masks_pred = None
            if triplets is None and boxes_gt is None:
                raise ValueError("generate: without triplets there is no graph to predict a layout from: pass boxes_gt")
            if model.has_graph and triplets is not None:      # a layout alone (split.generate_layouts): no encoder pass
                boxes_pred, masks_pred = model.sg_to_layout(objs, triplets, triplet_type, boxes_gt)[1:]
            if not model.has_image:
                return None, boxes_pred, masks_pred
            self._prepare()
            boxes = boxes_gt if boxes_gt is not None else boxes_pred
            masks = masks_gt if masks_gt is not None else masks_pred
            img, u8 = self._generator(objs, boxes.float().contiguous(), None if masks is None else masks.float().contiguous(),
                                      uint8, rescale, deprocess)
        return (u8 if uint8 else img), boxes_pred, masks_pred

    def generate_from_graphs(self, graphs, overlay=False, thickness=2, palette=None, labels=False, return_graph=False):
        """Authored scene graphs (authored.py: a list of graphs or the path of a JSON file) -> (images uint8 (B,3,H,W),
        boxes_pred (B,O,4), overlays uint8 (B,3,H,W) or None).  The graphs are encoded and checked on the host, uploaded
        once, and made canonical without boxes (`canonical_triplets(boxes=None)`: the authored rows are the location
        relations; converse and transitive edges and triplet_type as the model's learned_converse / learned_transitivity
        settings make them in training, converse draws from numpy's global stream as the data loader's).  The pictures come
        from `generate` on the predicted boxes, under its replay keys.  `overlay`: the pictures with the outlines of the
        predicted boxes, `thickness` pixels wide, row o in palette[o % P] — `palette` a sequence of RGB
        triples, by default authored.DEFAULT_PALETTE.  `labels` (needs `overlay`): the objects' names on the overlays as
        well (`ops.draw_labels_u8` on the outlined pictures, names by `authored.object_labels`).  `return_graph`: a fourth
        element (triplets (B,T,3), triplet_type (B,T)), the device tensors of the canonical graph the model was given —
        what `sgdraw.draw_scene_graphs` draws; the converse draws cannot be repeated afterwards."""
        from . import authored
        from .sg2im.data import canonical_triplets
        if labels and not overlay:
            raise ValueError("generate_from_graphs(labels=True) needs overlay=True: the names go on the layout pictures")
        if self.device.type != "cuda":
            raise RuntimeError(NO_CPU)
        vocab = self.opt.vocab
        graphs = authored.load_graphs(graphs, vocab)
        objs, rows, counts = authored.encode_graphs(graphs, vocab)
        conv_w = None
        if getattr(self.opt, "learned_converse", False):
            from .sg2im.model import get_conv_converse
            conv_w = get_conv_converse(self.model).detach().cpu().numpy()
        objs = objs.to(self.device)
        triplets, _, triplet_type = canonical_triplets(
            objs, None, None, counts, vocab, learned_transitivity=bool(getattr(self.opt, "learned_transitivity", False)),
            include_dummies=False, learned_converse=conv_w is not None, converse_weights=conv_w, triplets=rows)
        imgs, boxes_pred, _ = self.generate(objs, triplets, triplet_type)
        overlays = None
        if overlay:
            if imgs is None or boxes_pred is None:
                raise RuntimeError("generate_from_graphs(overlay=True) needs a model that predicts boxes and pictures")
            pal = torch.tensor(authored.DEFAULT_PALETTE if palette is None else palette, dtype=torch.uint8).reshape(-1, 3)
            pal, image_id = pal.to(self.device), vocab["object_name_to_idx"]["__image__"]
            overlays = ops.draw_boxes_u8(imgs, boxes_pred.detach().float(), objs, image_id, pal, thickness)
            if labels:
                overlays = ops.draw_labels_u8(overlays, boxes_pred.detach().float(), objs, image_id, pal,
                                              authored.object_labels(graphs))
        if return_graph:
            return imgs, boxes_pred, overlays, (triplets, triplet_type)
        return imgs, boxes_pred, overlays
