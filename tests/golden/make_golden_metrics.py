#!/usr/bin/env python3
"""Generate tests/golden/box_iou.npz by running the REAL reference's box metric on the CPU.

Runs only in the build container (needs /root/reference); nothing of the reference travels: the output is one `.npz` of
plain tensors + JSON metadata.  Usage:  python tests/golden/make_golden_metrics.py

What is recorded, per batch: the padded inputs a validation loop hands over (boxes_pred BEFORE the clamp of
scripts/train.py:196, boxes_gt, objs) and, scattered back to their (sample, object) slots, what
`jaccard(*remove_dummies_and_padding(boxes[i], objs[i], vocab, [clamp(boxes_pred[i], 0, 1), boxes[i]]))`
(scripts/train.py:203-217, sg2im/metrics.py:18-36, sg2im/utils.py:66-71) returns: iou (fp32), the mask of the rows it
kept, iou > 0.5 and iou > 0.3.  The aggregates are float64 sums of those per-object values.

The import shim is the one of make_golden.py.
"""
import json
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.dont_write_bytecode = True
sys.path.insert(0, REPO)
sys.path.insert(0, "/root/reference")


def _mod(name, **attrs):
    m = types.ModuleType(name)
    m.__dict__.update(attrs)
    sys.modules[name] = m
    return m


_mod("torch.tensor", Tensor=torch.Tensor)

from sg2im.metrics import jaccard  # noqa: E402  (reference)
from sg2im.utils import remove_dummies_and_padding  # noqa: E402  (reference)

from canonicalsg2im_amd.synth import BatchConfig, make_batch, make_vocab  # noqa: E402  (ours: inputs only)

NAN = float("nan")
HAND_IMAGE_ID = 7          # the hand-written batch uses a vocabulary whose __image__ is NOT 0: the two masks differ there


def reference_batch(boxes_pred, boxes, objs, vocab):
    """scripts/train.py:196-217 for one batch -> iou (B,O) fp32, counted / over05 / over03 (B,O) uint8."""
    B, O = objs.shape[:2]
    iou = np.zeros((B, O), np.float32)
    counted, o05, o03 = (np.zeros((B, O), np.uint8) for _ in range(3))
    clamped = torch.clamp(boxes_pred, 0., 1.)
    for i in range(B):
        rows = torch.arange(O)
        p, g, kept = remove_dummies_and_padding(boxes[i], objs[i], vocab, [clamped[i], boxes[i], rows])
        v, a, b = jaccard(p, g)
        kept = kept.numpy()
        iou[i, kept], counted[i, kept], o05[i, kept], o03[i, kept] = v, 1, a, b
    return iou, counted, o05, o03


def hand_batch():
    """(pred, gt, objs): one row per case the seeded batches do not hold."""
    I = HAND_IMAGE_ID
    rows = [
        # pred xywh                      gt xywh                          objs[.,0]   case
        ([0.10, 0.20, 0.30, 0.40], [0.10, 0.20, 0.30, 0.40], 3),      # identical boxes
        ([0.00, 0.00, 0.20, 0.20], [0.50, 0.50, 0.25, 0.25], 4),      # disjoint boxes
        ([0.30, 0.30, 0.00, 0.25], [0.25, 0.25, 0.50, 0.50], 5),      # zero-area prediction
        ([0.40, 0.40, 0.00, 0.00], [0.40, 0.40, 0.00, 0.00], 6),      # both of zero area: 0 / 0
        ([-0.25, 0.50, 1.50, 0.75], [0.00, 0.50, 0.75, 0.25], 2),     # prediction outside [0, 1] before the clamp
        ([0.10, 0.10, 0.50, 0.50], [0.10, 0.10, 0.50, 0.50], I),      # an __image__ row with a real box: not counted
        ([0.20, 0.20, 0.30, 0.30], [-1.0, -1.0, -1.0, -1.0], 9),      # a padded row (box of -1): not counted
        ([0.05, 0.15, 0.40, 0.35], [0.10, 0.10, 0.45, 0.30], 0),      # objs 0 with a real box: counted (not remove_dummy_objects)
        ([0.20, 0.20, 0.30, 0.30], [-1.0, 0.25, -1.0, -1.0], 8),      # one value differs from -1: counted
    ]
    pred = torch.tensor([r[0] for r in rows], dtype=torch.float32)
    gt = torch.tensor([r[1] for r in rows], dtype=torch.float32)
    objs = torch.tensor([[r[2]] for r in rows], dtype=torch.int64)
    # two samples: the first holds every case, the second the same rows reversed (and so a different order of summation)
    return torch.stack([pred, pred.flip(0)]), torch.stack([gt, gt.flip(0)]), torch.stack([objs, objs.flip(0)])


def aggregates(iou, counted, o05, o03):
    """(B,4) float64: sum of the kept rows' iou (a NaN among them makes it NaN), #(iou > 0.5), #(iou > 0.3), #kept."""
    kept = np.where(counted.astype(bool), iou, np.float32(0)).astype(np.float64)
    return np.stack([kept.sum(1), o05.astype(np.float64).sum(1), o03.astype(np.float64).sum(1),
                     counted.astype(np.float64).sum(1)], axis=1)


def main():
    vocab = make_vocab("coco")
    arrays, names = {}, []
    seeded = np.zeros(4)
    nan_seeded = 0
    for seed in range(8):
        batch = make_batch(vocab, BatchConfig(16, 64, 3, 8, "random"), seed=seed)
        objs, boxes = batch[1], batch[2]
        pred = (boxes + 0.15 * torch.randn(boxes.shape, generator=torch.Generator().manual_seed(seed))).clamp(0, 1)
        out = reference_batch(pred, boxes, objs, vocab)
        per = aggregates(*out)
        seeded += per.sum(0)
        nan_seeded += int(np.isnan(out[0]).sum())
        name = "seed%d" % seed
        names.append(name)
        for k, v in zip(("pred", "gt", "objs", "iou", "counted", "over05", "over03", "per_sample"),
                        (pred.numpy(), boxes.numpy(), objs.numpy()) + out + (per,)):
            arrays["%s_%s" % (name, k)] = v
    pred, gt, objs = hand_batch()
    out = reference_batch(pred, gt, objs, {"object_name_to_idx": {"__image__": HAND_IMAGE_ID}})
    names.append("hand")
    for k, v in zip(("pred", "gt", "objs", "iou", "counted", "over05", "over03", "per_sample"),
                    (pred.numpy(), gt.numpy(), objs.numpy()) + out + (aggregates(*out),)):
        arrays["hand_" + k] = v
    meta = {"ref": "scripts/train.py:196-217; sg2im/metrics.py:4-36; sg2im/utils.py:66-71", "batches": names,
            "image_id": {n: (HAND_IMAGE_ID if n == "hand" else vocab["object_name_to_idx"]["__image__"]) for n in names},
            "seeded": {"counted": int(seeded[3]), "over05": int(seeded[1]), "over03": int(seeded[2]), "nan": nan_seeded,
                       "sum_iou": float(seeded[0])},
            "per_sample": ["sum_iou", "over05", "over03", "counted"]}
    path = os.path.join(HERE, "box_iou.npz")
    np.savez(path, __meta__=np.frombuffer(json.dumps(meta).encode(), dtype=np.uint8), **arrays)
    print("box_iou.npz %.1f KB, %d arrays; seeded part: %s" % (os.path.getsize(path) / 1024, len(arrays), meta["seeded"]))
    print("hand iou:", arrays["hand_iou"][0], "counted:", arrays["hand_counted"][0])


if __name__ == "__main__":
    main()
