#!/usr/bin/env python3
"""Time one validation pass: `Evaluator.check_model` against the straightforward form assembled from the
package's other public pieces, on N images (batches of 16) at the C3 shapes, use_gt=True.  One measurement per process:

    python tools/eval_speed.py new|baseline [--samples 1024] [--warmup 2]

baseline = eval-mode `MetaGeneratorModel.forward(test_mode=True)` under no_grad, the same `gans_model` call, the
reference-style per-sample host loop for the IoU written in torch (remove_dummies_and_padding + jaccard + .cpu().numpy() per
sample, scripts/train.py:203-217), and the host `deprocess_batch` arithmetic for the five sample sets.
Prints one JSON line: {"mode", "samples", "seconds", "avg_iou"}; the pass is synchronised at both ends, after `--warmup`
batches of either form (kernel plans, weight layouts, allocator)."""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

MEAN, STD = [0.485, 0.456, 0.406], [0.229, 0.224, 0.225]


def deprocess_host(imgs):
    std1 = torch.as_tensor([1.0 / s for s in STD], dtype=torch.float32).view(3, 1, 1)
    mean2 = torch.as_tensor([-m for m in MEAN], dtype=torch.float32).view(3, 1, 1)
    out = []
    for i in range(imgs.size(0)):
        t = imgs[i].cpu().clone().div_(std1).sub_(mean2)
        lo, hi = t.min(), t.max()
        out.append(t.sub(lo).div(hi - lo)[None].mul(255).clamp(0, 255).byte())
    return torch.cat(out).permute(0, 2, 3, 1).numpy()


def jaccard(p, g):
    p = torch.stack([p[:, 0], p[:, 1], p[:, 0] + p[:, 2], p[:, 1] + p[:, 3]], 1)
    g = torch.stack([g[:, 0], g[:, 1], g[:, 0] + g[:, 2], g[:, 1] + g[:, 3]], 1)
    wh = torch.clamp(torch.min(p[:, 2:], g[:, 2:]) - torch.max(p[:, :2], g[:, :2]), min=0)
    inter = wh[:, 0] * wh[:, 1]
    iou = inter / ((p[:, 2] - p[:, 0]) * (p[:, 3] - p[:, 1]) + (g[:, 2] - g[:, 0]) * (g[:, 3] - g[:, 1]) - inter)
    return iou.cpu().numpy(), (iou > 0.5).cpu().numpy(), (iou > 0.3).cpu().numpy()


def baseline_check_model(tr, batches, image_id):
    model = tr.model
    model.eval()
    losses, total, t05, t03, boxes_n = {}, 0.0, 0.0, 0.0, 0.0
    with torch.no_grad():
        for batch in batches:
            imgs, objs, boxes, triplets, _, tt, masks, _ = batch
            out = model(objs, triplets, tt, boxes_gt=boxes, masks_gt=masks, test_mode=True)
            G = tr.gans_model(batch, out, mode="compute_generator_loss")
            bp = torch.clamp(out[1], 0., 1.)
            for i in range(boxes.size(0)):
                keep = (boxes[i] != -1).any(-1) & (objs[i, :, 0] != image_id)
                iou, a, b = jaccard(bp[i][keep], boxes[i][keep])
                total, t05, t03, boxes_n = total + iou.sum(), t05 + a.sum(), t03 + b.sum(), boxes_n + float(iou.shape[0])
            for k, v in G.items():
                losses.setdefault(k, []).append(v)
        samples = {"pred_box_pred_mask": model(objs, triplets, tt, test_mode=True)[0],
                   "pred_box_gt_mask": model(objs, triplets, tt, masks_gt=masks, test_mode=True)[0], "gt_img": imgs,
                   "gt_box_gt_mask": model(objs, triplets, tt, boxes_gt=boxes, masks_gt=masks, test_mode=True)[0],
                   "gt_box_pred_mask": model(objs, triplets, tt, boxes_gt=boxes, test_mode=True)[0]}
        samples = {k: deprocess_host(v) for k, v in samples.items()}
        mean = {k: float(torch.stack([x.mean() for x in v]).mean()) for k, v in losses.items() if k != "bbox_pred_all"}
    mean["avg_iou"] = total / boxes_n
    model.train()
    return mean, samples


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=["new", "baseline"])
    ap.add_argument("--samples", type=int, default=1024)
    ap.add_argument("--warmup", type=int, default=2)
    a = ap.parse_args()
    from canonicalsg2im_amd import train as T
    from canonicalsg2im_amd.evaluate import Evaluator
    from canonicalsg2im_amd.synth import BASELINE_CONFIGS, make_batch, make_vocab
    dev = torch.device("cuda:0")
    vocab = make_vocab("coco")
    opt = T.make_opt(vocab, ["--image_size", "256,256", "--no_vgg_loss", "--use_img_disc", "0", "--batch_size", "16"])
    torch.manual_seed(0)
    tr = T.Trainer(opt, dev)
    cfg = BASELINE_CONFIGS["C3"]["cfg"]
    n = -(-a.samples // 16)
    batches = [[None if t is None else t.to(dev) for t in make_batch(vocab, cfg, seed=1000 + i)] for i in range(n)]
    ev = Evaluator(tr)
    run = (lambda bs: ev.check_model(bs, use_gt=True, full_test=True)[:2]) if a.mode == "new" else \
        (lambda bs: baseline_check_model(tr, bs, vocab["object_name_to_idx"]["__image__"]))
    run(batches[:a.warmup])
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    mean, samples = run(batches)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    print(json.dumps({"mode": a.mode, "samples": n * 16, "seconds": round(dt, 4), "avg_iou": float(mean["avg_iou"]),
                      "total_loss": float(mean["total_loss"]), "sample_sets": len(samples)}), flush=True)


if __name__ == "__main__":
    main()
