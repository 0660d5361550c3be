"""Validation on a real MI355X (canonicalsg2im_amd/evaluate.py, csrc/metrics.hip): the box-IoU kernel against the fixture
recorded from the reference (bit for bit), `check_model` against the CPU oracle run through the same sequence of calls
(generator in eval mode, discriminators in training mode), the stale-weights trap, the survival of the trainer's captured
graphs, the sample pictures and the command line.

Tolerances.  Losses: rtol 1e-4, atol 1e-5 — what smoke() and the module tests use for losses.  iou: equality of bits.  Sums:
1e-12 relative to the float64 sum of the fixture's fp32 values (an ordered fp64 sum of a few thousand fp32 terms is exact to
~1e-16 per term).  Post-step parameters: the Adam bound of tests/test_gpu_graphs.py (2.2 * steps * lr per element)."""
import json
import os
import subprocess
import sys

import pytest
import torch

from conftest import ROOT, assert_close, load_golden
from test_gpu_sample import deprocess_host

pytestmark = pytest.mark.gpu

SMOKE = ["--image_size", "64,64", "--ngf", "4", "--ndf", "8", "--gconv_dim", "32", "--gconv_hidden_dim", "64",
         "--gconv_num_layers", "2", "--embedding_dim", "8", "--no_vgg_loss", "--batch_size", "2"]


@pytest.fixture(scope="module")
def cuda():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device("cuda:0")


def _same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


# --------------------------------------------------------------------------------------------- 1. the kernel
@pytest.mark.timeout(300)
def test_box_iou_equals_the_reference_bit_for_bit(cuda):
    from canonicalsg2im_amd import ops
    from canonicalsg2im_amd._lib import check, lib, ptr, stream
    meta, z = load_golden("box_iou")
    nan32 =lambda *s: torch.full(s, float("nan"), device=cuda)
    seen_nan = False
    for name in meta["batches"]:
        pred, gt, objs = z[name + "_pred"].to(cuda), z[name + "_gt"].to(cuda), z[name + "_objs"].to(cuda)
        want_iou, want_counted, want_per = z[name + "_iou"], z[name + "_counted"], z[name + "_per_sample"]
        B, O, A = objs.shape
        # first run: the library entry point itself, on outputs prefilled with NaN / 255; second run: the ops wrapper
        totals = torch.zeros(4, device=cuda, dtype=torch.float64)
        outs = (nan32(B, O), torch.full((B, O), 255, device=cuda, dtype=torch.uint8),
                torch.full((B, 4), float("nan"), device=cuda, dtype=torch.float64))
        check(lib.csg_box_iou(ptr(pred), ptr(gt), ptr(objs), B, O, A, meta["image_id"][name], ptr(outs[0]), ptr(outs[1]),
                              ptr(outs[2]), ptr(totals), stream()), "box_iou")
        runs = [outs + (totals,)]
        totals = torch.zeros(4, device=cuda, dtype=torch.float64)
        runs.append(ops.box_iou(pred, gt, objs, meta["image_id"][name], totals) + (totals,))
        torch.cuda.synchronize()
        iou, counted, per, totals = [t.cpu() for t in runs[0]]
        for a, b in zip(runs[0], runs[1]):
            assert a.dtype == b.dtype and torch.equal(a.cpu().view(torch.uint8), b.cpu().view(torch.uint8)), name + ": a second run differs"
        assert iou.dtype == torch.float32 and counted.dtype == torch.uint8 and per.dtype == torch.float64
        assert torch.equal(counted, want_counted), name
        assert _same_bits(iou.nan_to_num(nan=-7.0), want_iou.nan_to_num(nan=-7.0)), \
            "%s: %d of %d iou values differ from the reference's bits" % (name, int((iou != want_iou).sum()), iou.numel())
        assert torch.equal(torch.isnan(iou), torch.isnan(want_iou))
        assert not iou[counted == 0].any()
        seen_nan = seen_nan or bool(torch.isnan(iou).any())
        assert torch.equal(per[:, 1:], want_per[:, 1:]), name + ": threshold counts / counted"
        assert torch.equal(torch.isnan(per[:, 0]), torch.isnan(want_per[:, 0]))
        ok = ~torch.isnan(want_per[:, 0])
        rel = ((per[:, 0] - want_per[:, 0]).abs() / want_per[:, 0].abs().clamp_min(1e-300))[ok]
        print("%s: sum iou worst relative error %.3e" % (name, float(rel.max()) if rel.numel() else 0.0))
        assert (rel <= 1e-12).all(), name
        fold = want_per.sum(0)
        assert torch.equal(totals[1:], fold[1:])
        if not torch.isnan(fold[0]):
            assert abs(float(totals[0] - fold[0])) <= 1e-12 * abs(float(fold[0]))
        else:
            assert torch.isnan(totals[0])
    assert seen_nan, "the fixture's 0 / 0 row did not come out as NaN"


@pytest.mark.timeout(300)
def test_box_iou_totals_accumulate_over_batches(cuda):
    from canonicalsg2im_amd import ops
    meta, z = load_golden("box_iou")
    totals = torch.zeros(4, device=cuda, dtype=torch.float64)
    pers = []
    for name in ("seed0", "seed1"):
        pers.append(ops.box_iou(z[name + "_pred"].to(cuda), z[name + "_gt"].to(cuda), z[name + "_objs"].to(cuda),
                                meta["image_id"][name], totals)[2])
    torch.cuda.synchronize()
    # the fold is an ordered tree over the samples; (fold0 + fold1) in float64 of a few dozen O(1) terms: 1e-12 is far outside
    want = pers[0].cpu().sum(0) + pers[1].cpu().sum(0)
    assert torch.equal(totals.cpu()[1:], want[1:])
    assert abs(float(totals[0].cpu() - want[0])) <= 1e-12 * float(want[0])
    # shapes the library refuses, before any launch
    with pytest.raises(RuntimeError, match="csg_box_iou"):
        ops.box_iou(torch.zeros(1, 2, 4, device=cuda), torch.zeros(1, 2, 4, device=cuda),
                    torch.zeros(1, 2, 65, dtype=torch.int64, device=cuda), 0, totals)


@pytest.mark.timeout(300)
def test_box_iou_does_not_synchronise(cuda):
    from canonicalsg2im_amd import ops
    meta, z = load_golden("box_iou")
    pred, gt, objs = z["seed0_pred"].to(cuda), z["seed0_gt"].to(cuda), z["seed0_objs"].to(cuda)
    totals = torch.zeros(4, device=cuda, dtype=torch.float64)
    ops.box_iou(pred, gt, objs, 0, totals)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        live = False
        try:
            totals[0].item()
        except RuntimeError:
            live = True
        if live:
            ops.box_iou(pred, gt, objs, 0, totals)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    if not live:
        pytest.skip("torch.cuda.set_sync_debug_mode('error') does not raise on .item() with this torch build")


# --------------------------------------------------------------------------------------------- 2. check_model vs the oracle
def _trainer(cuda, extra, seed=0):
    from canonicalsg2im_amd import train as T
    from canonicalsg2im_amd.synth import make_vocab
    vocab = make_vocab("tiny")
    opt = T.make_opt(vocab, SMOKE + list(extra))
    torch.manual_seed(seed)
    tr = T.Trainer(opt, cuda)
    # a freshly initialised box head predicts boxes around 0 (negative sizes: every IoU is 0 after the clamp, and the metric
    # would be checked on zeros).  Centre its output on a plausible box, as a trained head's is, with half the initial spread.
    from canonicalsg2im_amd import ops
    with torch.no_grad():
        head = tr.model.sg_to_layout.module.box_net[2]
        head.bias.copy_(torch.tensor([0.25, 0.25, 0.4, 0.4]))
        head.weight.mul_(0.5)
    ops.invalidate_weight_caches()
    return vocab, opt, tr


def _val(vocab, seeds, B=2):
    from canonicalsg2im_amd.synth import BatchConfig, make_batch
    return [make_batch(vocab, BatchConfig(B, 64, 2, 5, "packed"), seed=s) for s in seeds]


def _dev(batches, cuda):
    return [[None if t is None else t.to(cuda) for t in b] for b in batches]


def _jaccard(pred, gt):
    """sg2im/metrics.py:4-36 restated (fp32, the reference's order)."""
    p = torch.stack([pred[:, 0], pred[:, 1], pred[:, 0] + pred[:, 2], pred[:, 1] + pred[:, 3]], 1)
    g = torch.stack([gt[:, 0], gt[:, 1], gt[:, 0] + gt[:, 2], gt[:, 1] + gt[:, 3]], 1)
    wh = torch.clamp(torch.min(p[:, 2:], g[:, 2:]) - torch.max(p[:, :2], g[:, :2]), min=0)
    inter = wh[:, 0] * wh[:, 1]
    area_p = (p[:, 2] - p[:, 0]) * (p[:, 3] - p[:, 1])
    area_g = (g[:, 2] - g[:, 0]) * (g[:, 3] - g[:, 1])
    return inter / (area_p + area_g - inter)


def _oracle_check_model(ts, batches, use_gt):
    """scripts/train.py:161-271 on the oracle: generator training=False, discriminators training=True, the same call order."""
    import oracle.functional as OF
    opt, vocab = ts.opt, ts.opt.vocab
    image_id = vocab["object_name_to_idx"]["__image__"]
    losses, ious = {}, []
    with torch.no_grad():
        for batch in batches:
            imgs, objs, boxes, triplets, _, tt = batch[:6]
            _, boxes_pred, _ = OF.sg2layout_forward(ts.sg, vocab, objs, triplets, tt)
            img = OF.generator_forward(ts.g, vocab, opt.image_size[0], objs, boxes if use_gt else boxes_pred, training=False,
                                       num_upsampling_layers=opt.num_upsampling_layers)
            G = OF.generator_losses(opt, ts.d, batch, (img, boxes_pred, None), training=True, dobj_state=ts.dobj,
                                    vgg_state=ts.vgg)
            for k, v in G.items():
                if k != "bbox_pred_all":
                    losses.setdefault(k, []).append(v.mean())
            clamped = torch.clamp(boxes_pred, 0., 1.)
            for i in range(objs.shape[0]):
                keep = (boxes[i] != -1).any(-1) & (objs[i, :, 0] != image_id)              # sg2im/utils.py:66-71
                ious.append(_jaccard(clamped[i][keep], boxes[i][keep]))
    out = {k: torch.stack(v).mean() for k, v in losses.items()}
    iou = torch.cat(ious).double()
    near = ((iou - 0.5).abs() <= 1e-5) | ((iou - 0.3).abs() <= 1e-5)
    assert not near.any(), "choose other seeds: an oracle IoU lies within 1e-5 of a threshold"
    out.update({"avg_iou": iou.sum() / iou.numel(), "total_iou_05": (iou > 0.5).double().sum() / iou.numel(),
                "total_iou_03": (iou > 0.3).double().sum() / iou.numel()})
    return out, iou


def _compare(got, want, tag):
    assert set(got) == set(want), (tag, sorted(got), sorted(want))
    assert not any(k.startswith("inception") for k in got)
    for k in want:
        a, b = float(got[k]), float(want[k])
        print("%s %-14s hip %.7f oracle %.7f  (diff %.2e)" % (tag, k, a, b, abs(a - b)))
    for k in want:
        a, b = float(got[k]), float(want[k])
        assert abs(a - b) <= 1e-4 * abs(b) + 1e-5, "%s %s: hip %g vs oracle %g" % (tag, k, a, b)


@pytest.mark.timeout(1200)
@pytest.mark.parametrize("use_img_disc", [1, 0])
def test_check_model_matches_the_oracle(cuda, use_img_disc):
    """Three validation batches, GT pass then PRED pass (the order the trainer runs them: the discriminators' u / v and
    BatchNorm statistics carry over from one pass to the next on both sides)."""
    import oracle
    from canonicalsg2im_amd import train as T
    from canonicalsg2im_amd.evaluate import Evaluator
    vocab, opt, tr = _trainer(cuda, ["--use_img_disc", str(use_img_disc)])
    tr.step(_dev(_val(vocab, [3]), cuda)[0])                      # running statistics and u / v off their initial values
    torch.cuda.synchronize()
    ts = T.oracle_state_from(tr, oracle)
    val = _val(vocab, [101, 102, 103])
    ev = Evaluator(tr)
    before = {k: v.detach().clone() for k, v in tr.model.state_dict().items()}
    for use_gt in (True, False):
        got, samples, table = ev.check_model(_dev(val, cuda), use_gt=use_gt, num_val_samples=6)
        want, iou = _oracle_check_model(ts, val, use_gt)
        _compare(got, want, "use_img_disc=%d use_gt=%s" % (use_img_disc, use_gt))
        assert float(want["avg_iou"]) > 0.05 and 0.0 < float(want["total_iou_03"]) < 1.0, "the metric is checked on trivial boxes"
        assert tr.model.training and tr.discriminator.training
        assert table["image_id"].tolist() == [0, 1] * 3 and int(table["num_boxes"].sum()) == iou.numel()
        assert table["number_of_objects"].tolist() == [b[1].shape[1] for b in val for _ in range(2)]
        counted = table["counted"].bool()
        assert_close(table["iou"][counted], iou.float(), 1e-4, 1e-5, "per-object iou")
        assert_close(table["iou05"], torch.stack([(table["iou"][i][counted[i]] > 0.5).double().mean() for i in range(6)]), 0, 0,
                     "iou05 is the share above 0.5")
        assert set(samples) == {"pred_box_pred_mask", "pred_box_gt_mask", "gt_img", "gt_box_gt_mask", "gt_box_pred_mask"}
    # the generator and the encoder are untouched by validation
    after = tr.model.state_dict()
    for k in before:
        assert torch.equal(before[k], after[k]), "validation changed model entry %s" % k
    # num_val_samples stops the loop (2 images per batch): the third batch is not consumed
    seen = []

    def feed():
        for b in _dev(val, cuda):
            seen.append(1)
            yield b
    _, _, table = ev.check_model(feed(), use_gt=True, num_val_samples=3)
    assert len(seen) == 2 and table["image_id"].numel() == 4
    _, _, table = ev.check_model(feed(), use_gt=True, num_val_samples=3, full_test=True)
    assert table["image_id"].numel() == 6


@pytest.mark.timeout(1200)
def test_a_training_step_between_two_validations_is_seen(cuda):
    """check_model -> two trainer steps -> check_model: the fused Adam step and a replayed step write weights and running
    statistics without bumping `_version`; a sampler holding the first call's preparation would repeat the first call."""
    import oracle
    from canonicalsg2im_amd import train as T
    from canonicalsg2im_amd.evaluate import Evaluator
    vocab, opt, tr = _trainer(cuda, ["--use_img_disc", "1"])
    ts = T.oracle_state_from(tr, oracle)
    val, steps = _val(vocab, [201, 202, 203]), _val(vocab, [11, 12])
    ev = Evaluator(tr)
    first, _, _ = ev.check_model(_dev(val, cuda), use_gt=True)
    want_first, _ = _oracle_check_model(ts, val, True)
    _compare(first, want_first, "before the steps")
    for b in steps:
        tr.step(_dev([b], cuda)[0])
        oracle.train_step(ts, b)
    second, _, _ = ev.check_model(_dev(val, cuda), use_gt=True)
    want_second, _ = _oracle_check_model(ts, val, True)
    for k in ("GAN_Img", "GAN_Feat", "total_loss"):
        a, b = float(first[k]), float(second[k])
        print("%-10s first %.7f second %.7f" % (k, a, b))
        assert abs(a - b) > 1e-4 * abs(a) + 1e-5, "%s did not move over two training steps: stale weights" % k
    _compare(second, want_second, "after two steps")


@pytest.mark.timeout(1200)
def test_captured_step_graphs_survive_a_validation(cuda):
    import oracle
    from canonicalsg2im_amd import train as T
    from canonicalsg2im_amd.evaluate import Evaluator
    vocab, opt, tr = _trainer(cuda, ["--use_img_disc", "1"])
    assert tr.graphs is not None
    ts = T.oracle_state_from(tr, oracle)
    steps, val = _val(vocab, [21, 22, 23, 24]), _val(vocab, [301, 302, 303])
    ev = Evaluator(tr)
    for b in steps[:3]:
        tr.step(_dev([b], cuda)[0])
        oracle.train_step(ts, b)
    g = tr.graphs
    assert (g.captures, g.replays, g.eager_steps) == (1, 2, 1)
    got, _, _ = ev.check_model(_dev(val, cuda), use_gt=True)
    want, _ = _oracle_check_model(ts, val, True)
    assert tr.model.training
    G, D = tr.step(_dev([steps[3]], cuda)[0])
    Go, Do, _ = oracle.train_step(ts, steps[3])
    torch.cuda.synchronize()
    assert (g.captures, g.replays, g.eager_steps) == (1, 3, 1), (g.captures, g.replays, g.eager_steps)
    assert g.sets and tr.model.training
    _compare(got, want, "validation between replays")
    for k in ("bbox_pred", "GAN_Img", "GAN_Feat", "total_loss"):
        print("step after validation %-10s hip %.7f oracle %.7f" % (k, float(G[k]), float(Go[k].detach())))
    # post-step state against the oracle's train_step x3 / evaluate / train_step: tests/test_gpu_graphs.py's Adam bound
    snap = T.state_snapshot(tr)
    lr, n = 1e-4, 4
    worst = 0.0
    for part, ref in (("sg", ts.sg), ("g", ts.g), ("d", ts.d)):
        for k, v in ref.items():
            if not (torch.is_tensor(v) and v.requires_grad):
                continue
            d = float((snap[part][k].float() - v.detach()).abs().max())
            worst = max(worst, d / (1e-2 if "candidates_weights" in k else lr))
            assert d <= 2.2 * n * (1e-2 if "candidates_weights" in k else lr), "%s.%s differs by %g" % (part, k, d)
    print("post-step parameters: worst difference %.2f learning rates (bound %.1f)" % (worst, 2.2 * n))


# --------------------------------------------------------------------------------------------- 3. samples
@pytest.mark.timeout(1200)
def test_samples_are_the_samplers_pictures(cuda):
    from canonicalsg2im_amd.evaluate import Evaluator
    vocab, opt, tr = _trainer(cuda, ["--use_img_disc", "1"])
    tr.step(_dev(_val(vocab, [5]), cuda)[0])
    val = _dev(_val(vocab, [401, 402]), cuda)
    ev = Evaluator(tr)
    _, samples, _ = ev.check_model(val, use_gt=False)
    imgs, objs, boxes, triplets, _, tt, masks, _ = val[-1]
    assert masks is None and opt.mask_size == 0
    assert samples["pred_box_pred_mask"] is samples["pred_box_gt_mask"]
    assert samples["gt_box_gt_mask"] is samples["gt_box_pred_mask"]
    s = ev.sampler
    want = {"pred_box_pred_mask": s.generate(objs, triplets, tt)[0], "pred_box_gt_mask": s.generate(objs, triplets, tt, masks_gt=masks)[0],
            "gt_box_gt_mask": s.generate(objs, triplets, tt, boxes_gt=boxes, masks_gt=masks)[0],
            "gt_box_pred_mask": s.generate(objs, triplets, tt, boxes_gt=boxes)[0]}
    tr.model.train()
    for k, v in samples.items():
        assert v.dtype == torch.uint8 and tuple(v.shape) == (2, 64, 64, 3) and not v.is_cuda, k
    for k, w in want.items():
        assert torch.equal(samples[k], w.permute(0, 2, 3, 1).cpu()), k
    assert torch.equal(samples["gt_img"], deprocess_host(imgs, True).permute(0, 2, 3, 1))
    assert not torch.equal(samples["gt_box_gt_mask"], samples["pred_box_pred_mask"])


# --------------------------------------------------------------------------------------------- 4. command line
@pytest.mark.timeout(1200)
def test_command_line_prints_both_passes_and_writes_the_files(cuda, tmp_path):
    from canonicalsg2im_amd.evaluate import Evaluator
    from canonicalsg2im_amd.scripts import evaluate as cli
    argv = SMOKE + ["--use_img_disc", "1", "--dataset", "coco", "--num_val_samples", "4"]
    from canonicalsg2im_amd import train as T
    from canonicalsg2im_amd.synth import make_vocab
    opt = T.make_opt(make_vocab("coco"), argv)
    torch.manual_seed(1)
    tr = T.Trainer(opt, cuda)
    from canonicalsg2im_amd.synth import BatchConfig, make_batch
    tr.step([None if t is None else t.to(cuda) for t in make_batch(opt.vocab, BatchConfig(2, 64, 3, 8, "random"), seed=1)])
    ck = tmp_path / "itr_1.pt"
    tr.save_checkpoint(str(ck), t=1)
    out = tmp_path / "val"
    r = subprocess.run([sys.executable, "-m", "canonicalsg2im_amd.scripts.evaluate"] + argv +
                       ["--checkpoint_name", str(ck), "--output_dir", str(out)], cwd=ROOT, env=dict(os.environ, PYTHONPATH=ROOT),
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("Iter: 1, ")]
    assert len(lines) == 2 and "GT VAL avg_iou:" in lines[0] and lines[1].startswith("Iter: 1, VAL avg_iou:"), r.stdout
    metrics = json.load(open(out / "metrics.json"))
    table = json.load(open(out / "table.json"))
    assert len(table["image_id"]) == 4 and len(table["iou"]) == 4
    pngs = sorted(p.name for p in out.glob("*.png"))
    assert len(pngs) == 5 * 2 and "val_gt_img_000.png" in pngs, pngs
    # the same two passes in this process, from the same checkpoint
    tr2 = T.Trainer(opt, cuda)
    tr2.load_checkpoint(str(ck))
    ev = Evaluator(tr2)
    gt_losses, _, _ = ev.check_model(cli.validation_batches(opt, tr2, cuda), use_gt=True)
    losses, _, _ = ev.check_model(cli.validation_batches(opt, tr2, cuda), use_gt=False)
    assert metrics["GT VAL"]["avg_iou"] == float(gt_losses["avg_iou"]) and metrics["VAL"]["avg_iou"] == float(losses["avg_iou"])
    assert_close(torch.tensor(metrics["VAL"]["total_loss"]), losses["total_loss"].double(), 1e-4, 1e-5, "VAL total_loss")
