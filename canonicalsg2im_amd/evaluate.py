"""Validation of a model in training: the reference's `check_model` (scripts/train.py:161-271, called for the `GT VAL` and
`VAL` lines at :404-429) on the device.

`Evaluator(trainer).check_model(batches, use_gt)` puts the trainer's generator in eval mode and, under `no_grad`, per batch:
runs the scene-graph encoder, walks the generator on the inference kernels (`sample.Sampler` ADOPTING the trainer's own
`MetaGeneratorModel`: one copy of the weights) on the ground-truth boxes / masks (`use_gt=True`) or on the predicted ones,
calls `trainer.gans_model(batch, model_out, mode="compute_generator_loss")`, and measures the box IoU of the predicted layout
(`ops.box_iou`: jaccard behind remove_dummies_and_padding, sg2im/metrics.py:18-36, sg2im/utils.py:66-71).  It returns the
reference's triple `(mean_losses, samples, table)`.

As in the reference only `model.eval()` is called (:162): the discriminators stay in TRAINING mode, so a validation pass
advances their spectral-norm u / v and moves the object discriminator's BatchNorm running statistics, exactly as the
reference's validation does.  The generator, the encoder and every optimiser are left as they were, and `model.train()`
is called at the end (:270), also when an error is raised — errors are raised, not swallowed (the reference prints them
and goes on, :239-240).

Nothing is read back inside the loop by this module: loss values, the metric's running totals and the per-image table stay
on the device and come to the host in ONE copy at the end.  (`gans_model` itself reads the list of real objects for the
object discriminator's crops, as it does in a training step.)  The trainer's captured step graphs are not touched.

Differences from the reference, on purpose:
  * `inception_mean` / `inception_std` appear only when `check_model` is given an Inception network (`inception=`,
    `scripts.evaluate --inception_weights FILE`): every generated batch is then fed to `quality.InceptionScore` as at :198 and
    the score is computed with splits=5 (:262-268).  Without a network the two keys are absent — the reference's weights are a
    download, and a zero there would be a false number;
  * the table's `iou05` is the share of boxes above 0.5; the reference appends `mean(iou03)` under that name (:221), a slip;
  * the table is a dict of host tensors, not a pandas frame (pandas is not a dependency); `predicted_boxes` / `gt_boxes`
    are the padded (N, O, 4) arrays with `counted` marking the rows the metric kept, not strings; no `class` column;
  * `jaccard_masks` is commented out in the reference's loop (:204-214) and absent here.

With a process group up, every rank evaluates the batches IT is given and the results are rank-local: `check_model` issues
no collective.  Multi-GPU evaluation (sharding a validation set, reducing the totals) is out of scope.
"""
import torch

from . import ops
from .sample import NO_CPU, Sampler

_SAMPLE_KEYS = ("pred_box_pred_mask", "pred_box_gt_mask", "gt_img", "gt_box_gt_mask", "gt_box_pred_mask")


def _fetch(tensors):
    """{name: device tensor} -> {name: host tensor}, every byte in ONE device-to-host copy."""
    names = [k for k, t in tensors.items() if t.numel()]
    if not names:
        return {k: t.cpu() for k, t in tensors.items()}
    dev = tensors[names[0]].device
    parts, spans, off = [], {}, 0
    for k in names:
        raw = tensors[k].contiguous().view(-1).view(torch.uint8)
        pad = (-raw.numel()) % 8                        # every slice starts on an 8-byte boundary of the host buffer
        spans[k] = (off, raw.numel())
        parts.append(raw)
        if pad:
            parts.append(torch.zeros(pad, dtype=torch.uint8, device=dev))
        off += raw.numel() + pad
    host = torch.cat(parts).cpu()
    out = {}
    for k, t in tensors.items():
        if k in spans:
            o, n = spans[k]
            out[k] = host[o:o + n].view(t.dtype).view(t.shape)
        else:
            out[k] = torch.empty(t.shape, dtype=t.dtype)
    return out


def _pad_rows(t, O, value):
    """(B, o, ...) -> (B, O, ...) with `value` in the added rows."""
    if t.shape[1] == O:
        return t
    out = t.new_full((t.shape[0], O) + tuple(t.shape[2:]), value)
    out[:, :t.shape[1]] = t
    return out


class Evaluator:
    def __init__(self, trainer):
        if torch.device(trainer.device).type != "cuda":
            raise RuntimeError(NO_CPU)
        self.trainer = trainer
        self.opt = trainer.opt
        self.sampler = Sampler(trainer.opt, trainer.device, model=trainer.model)
        self._epoch = None                       # ops.weight_epoch() the sampler's preparation was made at
        self.image_id = trainer.opt.vocab["object_name_to_idx"]["__image__"]

    def _fresh_sampler(self):
        """The sampler's preparation (W / sigma, packed operands, eval statistics) is derived from weights a training step
        rewrites WITHOUT bumping `_version` (fused Adam; a replayed step).  `ops.weight_epoch()` advances with every
        optimiser step, replayed ones included: a preparation of another epoch is dropped here."""
        epoch = ops.weight_epoch()
        if epoch != self._epoch:
            self.sampler.invalidate()
            self._epoch = epoch

    def _walk(self, objs, boxes, masks):
        return self.sampler._generator(objs, boxes.float().contiguous(), None if masks is None else masks.float().contiguous(),
                                       False, True)[0]

    def check_model(self, batches, use_gt=True, num_val_samples=None, full_test=False, inception=None):
        """-> (mean_losses, samples, table).  `batches`: an iterable of collated batches on the trainer's device.
        `inception`: an `inception.InceptionV3("torchvision", ...)`; mean_losses then gains `inception_mean` /
        `inception_std` of the generated images (splits=5), and `inception_stand_in` = 1.0 when the network is the seeded
        stand-in, whose score means nothing.
        mean_losses: {name: 0-d host tensor} — every generator loss but `bbox_pred_all`, averaged per batch and then over
        the batches, plus `avg_iou`, `total_iou_05`, `total_iou_03` (totals / counted boxes, float64) with the graph model.
        samples: {key: uint8 (B,H,W,3) host tensor} of the LAST batch (keys and conditions of :242-255).
        table: {column: host tensor} with one row per validated image (see the module docstring).
        Stops after `num_val_samples` images (default: --num_val_samples) unless `full_test`."""
        tr, opt, model = self.trainer, self.opt, self.trainer.model
        limit = opt.num_val_samples if num_val_samples is None else num_val_samples
        dev = torch.device(tr.device)
        obj_d = None if opt.use_img_disc or opt.skip_generation else tr.discriminator.obj_discriminator
        losses, rows = {}, []
        score = None
        if inception is not None:
            from .quality import InceptionScore
            score = InceptionScore(inception)
        totals = torch.zeros(4, device=dev, dtype=torch.float64)
        num_samples, last = 0, None
        self._fresh_sampler()
        model.eval()
        try:
            with torch.no_grad():
                if model.has_image:
                    self.sampler._prepare()
                for batch in batches:
                    imgs, objs, boxes, triplets, _, triplet_type, masks, image_ids = batch
                    if not objs.is_cuda:
                        raise RuntimeError(NO_CPU)
                    boxes_pred = masks_pred = img = None
                    if model.has_graph:
                        boxes_pred, masks_pred = model.sg_to_layout(objs, triplets, triplet_type, boxes if use_gt else None)[1:]
                    if model.has_image:
                        if use_gt:                   # ground truth wins wherever it is given (sg2im/meta_models.py:47-49)
                            img = self._walk(objs, boxes, masks if masks is not None else masks_pred)
                        else:
                            img = self._walk(objs, boxes_pred, masks_pred)
                    if obj_d is not None:
                        obj_d.prefetch_index(objs)
                    G = tr.gans_model(batch, (img, boxes_pred, masks_pred), mode="compute_generator_loss")
                    if obj_d is not None:
                        obj_d.release_index()
                    if score is not None and img is not None:
                        score.update(img.float())            # scripts/train.py:198
                    for k, v in G.items():
                        if k != "bbox_pred_all":
                            losses.setdefault(k, []).append(v.mean())
                    if model.has_graph:
                        iou, counted, per = ops.box_iou(boxes_pred, boxes, objs, self.image_id, totals)
                        ids = torch.as_tensor(image_ids).to(dev, non_blocking=True) if not torch.is_tensor(image_ids) \
                            else image_ids.to(dev, non_blocking=True)
                        rows.append((ids.reshape(-1).to(torch.int64), per, iou, counted,
                                     torch.clamp(boxes_pred.detach().float(), 0., 1.), boxes.float()))
                    last = batch
                    num_samples += int(imgs.shape[0])
                    if not full_test and limit and num_samples >= limit:
                        break
                if last is None:
                    raise ValueError("check_model: no validation batch was given")
                samples = self._samples(last)
                mean_losses, table = self._collect(losses, totals, rows, dev)
                if score is not None and score.n:
                    mean, std = score.compute(splits=5)     # scripts/train.py:266
                    mean_losses.update({"inception_mean": torch.tensor(mean, dtype=torch.float64),
                                        "inception_std": torch.tensor(std, dtype=torch.float64)})
                    if score.stand_in:
                        mean_losses["inception_stand_in"] = torch.tensor(1.0, dtype=torch.float64)
        finally:
            model.train()                               # scripts/train.py:270
        return mean_losses, samples, table

    # ------------------------------------------------------------------ samples (scripts/train.py:242-255)
    def _samples(self, batch):
        opt = self.opt
        if opt.skip_generation:
            return {}
        imgs, objs, boxes, triplets, _, triplet_type, masks, _ = batch
        gen = lambda **kw: self.sampler.generate(objs, triplets, triplet_type, **kw)[0]
        dev = {}
        if not opt.skip_graph_model:
            dev["pred_box_pred_mask"] = gen()
            # without masks (mask_size == 0) the two calls have identical inputs: generated once, shared
            dev["pred_box_gt_mask"] = gen(masks_gt=masks) if masks is not None else dev["pred_box_pred_mask"]
        dev["gt_img"] = ops.deprocess_u8(imgs.float().contiguous(memory_format=torch.channels_last), True)
        dev["gt_box_gt_mask"] = gen(boxes_gt=boxes, masks_gt=masks)
        dev["gt_box_pred_mask"] = gen(boxes_gt=boxes) if masks is not None else dev["gt_box_gt_mask"]
        unique = {}
        for k, v in dev.items():
            unique.setdefault(id(v), v.permute(0, 2, 3, 1))
        host = _fetch({str(i): v for i, v in unique.items()})
        return {k: host[str(id(dev[k]))] for k in _SAMPLE_KEYS if k in dev}

    # ------------------------------------------------------------------ one copy to the host
    def _collect(self, losses, totals, rows, dev):
        names = list(losses)
        pack = {"totals": totals}
        if names:
            pack["losses"] = torch.stack([torch.stack(losses[k]).mean() for k in names]).float()
        if rows:
            O = max(r[2].shape[1] for r in rows)
            pack["image_id"] = torch.cat([r[0] for r in rows])
            pack["per_sample"] = torch.cat([r[1] for r in rows])
            pack["number_of_objects"] = torch.cat([torch.full((r[2].shape[0],), r[2].shape[1], dtype=torch.int64, device=dev)
                                                   for r in rows])
            pack["iou"] = torch.cat([_pad_rows(r[2], O, 0.0) for r in rows])
            pack["counted"] = torch.cat([_pad_rows(r[3], O, 0) for r in rows])
            pack["predicted_boxes"] = torch.cat([_pad_rows(r[4], O, -1.0) for r in rows])
            pack["gt_boxes"] = torch.cat([_pad_rows(r[5], O, -1.0) for r in rows])
        host = _fetch(pack)
        mean_losses = {k: host["losses"][i].clone() for i, k in enumerate(names)}
        table = {}
        if rows:
            t = host["totals"]
            mean_losses.update({"avg_iou": t[0] / t[3], "total_iou_05": t[1] / t[3], "total_iou_03": t[2] / t[3]})
            per = host["per_sample"]
            table = {"image_id": host["image_id"], "avg_iou": per[:, 0] / per[:, 3], "iou03": per[:, 2] / per[:, 3],
                     "iou05": per[:, 1] / per[:, 3], "num_boxes": per[:, 3].clone(),
                     "number_of_objects": host["number_of_objects"], "iou": host["iou"], "counted": host["counted"],
                     "predicted_boxes": host["predicted_boxes"], "gt_boxes": host["gt_boxes"]}
        return mean_losses, table
