"""The split walk on a real MI355X (canonicalsg2im_amd/split.py): the `decode_img` constants of csg_deprocess_u8 against
torch's fp32 host arithmetic, and `generate_split` / `generate_layouts` over the tiny dataset folders against the calls they
are made of (`Sampler.generate`, `ops.deprocess_u8`, `ops.draw_boxes_u8`, `ops.box_iou`) on the batches of a second builder
with the same seed, and against `Evaluator.check_model`.

No tolerance anywhere: the walk orders existing launches, so what it writes equals what those launches give, byte for byte
and bit for bit; the PNG files are lossless.  The expected pictures are computed with graph capture off: every batch of
the walk — the eager one, the capturing one, the replayed ones and the partial one — is compared with an eager call.
Shapes: 64 x 64 pictures, `--ngf 8`, folders of five (Visual Genome: four) pictures in batches of two."""
import json
import os
import random
import re

import numpy as np
import pytest
import torch

import clevr_cases as cc
import pair_cases as pc
import vg_cases as vc
from test_gpu_coco_pairs import MODEL

pytestmark = pytest.mark.gpu

ALL_SETS = ["gt", "generation/gt_box_gt_mask", "generation/pred_box_pred_mask", "layout/gt", "layout/pred"]
BOX_BIAS = [0.2, 0.25, 0.45, 0.4]          # the untrained box head's last bias: boxes with an area, IoU above 0 (test_gpu_authored.py)


@pytest.fixture(scope="module")
def cuda():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device("cuda:0")


# --------------------------------------------------------------------------------------------- 1. decode_img
def decode_img_host(imgs, rescale):
    """deprocess_batch(imgs, rescale, decode_img) of sg2im/data/utils.py:17-24, :46-65 on fp32 CPU tensors: T.Normalize is
    sub_(mean).div_(std) in place, twice; rescale over the whole image; mul(255).clamp(0, 255).byte()."""
    out = []
    for i in range(imgs.size(0)):
        t = imgs[i].clone()
        t.sub_(torch.zeros(3, 1, 1)).div_(torch.full((3, 1, 1), 2.0))
        t.sub_(torch.full((3, 1, 1), -0.5)).div_(torch.ones(3, 1, 1))
        if rescale:
            lo, hi = t.min(), t.max()
            t = t.sub(lo).div(hi - lo)
        out.append(t[None].mul(255).clamp(0, 255).byte())
    return torch.cat(out, dim=0)


@pytest.mark.timeout(300)
@pytest.mark.parametrize("rescale", [True, False])
@pytest.mark.parametrize("hw", [(64, 64), (12, 20)])
@pytest.mark.parametrize("B", [1, 3])
def test_decode_img_equals_the_host_arithmetic_byte_for_byte(cuda, B, hw, rescale):
    from canonicalsg2im_amd import ops
    H, W = hw
    g = torch.Generator().manual_seed(1000 * B + H + int(rescale))
    x = torch.randn((B + 1, 3, H, W), generator=g) * 1.5             # B images beyond [-1, 1] ...
    x[B] = torch.where(torch.rand((3, H, W), generator=g) < 0.5, -1.0, 1.0)         # ... and one holding exactly -1 and +1,
    assert set(x[B].unique().tolist()) == {-1.0, 1.0} and float(x[:B].abs().max()) > 3.0
    pm = ops.deprocess_u8(x[B:].to(cuda).contiguous(memory_format=torch.channels_last), rescale, "decode_img")
    assert torch.equal(pm.cpu(), decode_img_host(x[B:], rescale)) and set(pm.unique().tolist()) == {0, 255}
    if B > 1:                                                        # on its own above, and as the batch's last image
        x[B - 1] = x[B]
    x = x[:B]
    want = decode_img_host(x, rescale)
    dev = x.to(cuda).contiguous(memory_format=torch.channels_last)
    got = ops.deprocess_u8(dev, rescale, deprocess="decode_img")
    again = ops.deprocess_u8(dev, rescale, "decode_img")
    torch.cuda.synchronize()
    differing = int((got.cpu() != want).sum())
    print("decode_img B=%d %dx%d rescale=%s: %d differing bytes of %d" % (B, H, W, rescale, differing, want.numel()))
    assert got.dtype == torch.uint8 and tuple(got.shape) == (B, 3, H, W) and differing == 0
    assert torch.equal(got, again)
    if B > 1:
        assert torch.equal(got[B - 1], pm[0])                        # -1 -> 0 and +1 -> 255, with and without rescale
    named, plain, positional = ops.deprocess_u8(dev, rescale, deprocess="imagenet"), ops.deprocess_u8(dev, rescale), \
        ops.deprocess_u8(dev) if rescale else ops.deprocess_u8(dev, False)
    assert torch.equal(named, plain) and torch.equal(plain, positional) and not torch.equal(named, got)
    with pytest.raises(ValueError, match="'imagenet' or 'decode_img'.*'srgb'"):
        ops.deprocess_u8(dev, rescale, deprocess="srgb")


# --------------------------------------------------------------------------------------------- 2. a folder, walked and expected
def _opt(root, extra):
    from canonicalsg2im_amd import train as T
    from canonicalsg2im_amd.scripts.train import build_parser, folder_dataset
    argv = MODEL + ["--batch_size", "2", "--dataroot", root] + list(extra)
    ds = folder_dataset(build_parser().parse_args(argv), "val")
    assert ds is not None
    return ds, T.make_opt(ds.vocab, argv)


def _checkpoint(opt, cuda, seed=5):
    """A seeded trainer whose box head predicts boxes with an area, and its checkpoint on the host."""
    from canonicalsg2im_amd import train as T
    torch.manual_seed(seed)
    trainer = T.Trainer(opt, cuda)
    if trainer.model.has_graph:
        named = dict(trainer.model.named_parameters())
        last = sorted((k for k in named if re.search(r"box_net\.\d+\.bias$", k)),
                      key=lambda k: int(re.search(r"box_net\.(\d+)\.", k).group(1)))[-1]
        assert tuple(named[last].shape) == (4,)
        with torch.no_grad():
            named[last].copy_(torch.tensor(BOX_BIAS))
    ckpt = {k: ({n: t.detach().cpu().clone() for n, t in v.items()} if k.endswith("_state") and "optim" not in k else v)
            for k, v in trainer.checkpoint_dict(3, 0).items()}
    return trainer, ckpt


def _batches(ds, opt, owner, cuda, batch_size=2):
    """The split's batches in file order from a builder of its own, seeded as scripts/sample.py seeds it."""
    from canonicalsg2im_amd.scripts.train import folder_builder
    from canonicalsg2im_amd.sg2im.data.loader import file_order_batches
    builder = folder_builder(ds, opt, owner, cuda, rng=random.Random(0))
    try:
        yield from builder.batches(file_order_batches(len(ds), batch_size))
    finally:
        builder.close()


def _expected(sampler, batches, deprocess, cuda):
    """Per batch what the existing calls give, with graph capture off -> ([{set: uint8 (B,3,H,W)}], [rows' tensors], totals)."""
    from canonicalsg2im_amd import authored, graphs, ops
    image_id = sampler.opt.vocab["object_name_to_idx"]["__image__"]
    pal = torch.tensor(authored.DEFAULT_PALETTE, dtype=torch.uint8).to(cuda)
    totals = torch.zeros(4, device=cuda, dtype=torch.float64)
    pics, facts = [], []
    replays = sampler.replays
    was, graphs.ENABLED = graphs.ENABLED, False
    try:
        for imgs, objs, boxes, trip, _, tt, masks, ids in batches:
            p = {"generation/gt_box_gt_mask": sampler.generate(objs, trip, tt, boxes_gt=boxes, masks_gt=masks, deprocess=deprocess)[0],
                 "gt": ops.deprocess_u8(imgs.float().contiguous(memory_format=torch.channels_last), True, deprocess)}
            p["layout/gt"] = ops.draw_boxes_u8(p["gt"], boxes.float(), objs, image_id, pal, 2)
            f = {"ids": ids.cpu().tolist(), "objs": objs.cpu(), "boxes": boxes.float().cpu()}
            if sampler.model.has_graph:
                p["generation/pred_box_pred_mask"], boxes_pred, _ = sampler.generate(objs, trip, tt, deprocess=deprocess)
                p["layout/pred"] = ops.draw_boxes_u8(p["generation/pred_box_pred_mask"], boxes_pred.float(), objs, image_id, pal, 2)
                iou, counted, _ = ops.box_iou(boxes_pred, boxes, objs, image_id, totals)
                f.update(boxes_pred=boxes_pred.float().cpu(), iou=iou.cpu(), counted=counted.cpu().bool())
            pics.append({k: v.cpu() for k, v in p.items()})
            facts.append(f)
    finally:
        graphs.ENABLED = was
    torch.cuda.synchronize()
    assert sampler.replays == replays
    return pics, facts, totals.cpu()


def _decoded(path):
    from PIL import Image
    with Image.open(path) as im:
        assert im.mode == "RGB"
        return torch.from_numpy(np.asarray(im).copy()).permute(2, 0, 1)


def _check_files(out, pics, facts, sets):
    """Exactly the expected ids in exactly the expected sets, every decoded file equal to the expected picture."""
    ids = [i for f in facts for i in f["ids"]]
    found = sorted(os.path.relpath(os.path.join(d, n), out).replace(os.sep, "/") for d, _, names in os.walk(out) for n in names)
    assert found == sorted(["layouts.json"] + ["%s/%d.png" % (s, i) for s in sets for i in ids]), found
    for p, f in zip(pics, facts):
        for s in sets:
            for b, i in enumerate(f["ids"]):
                got = _decoded(os.path.join(out, s, "%d.png" % i))
                assert torch.equal(got, p[s][b]), "%s/%d.png: %d bytes differ" % (s, i, int((got != p[s][b]).sum()))
    return ids


def _bits(rows_of_floats):
    return torch.tensor(rows_of_floats, dtype=torch.float64).to(torch.float32).reshape(-1).view(torch.int32)


def _check_rows(rows, facts, vocab):
    from canonicalsg2im_amd import authored
    image_id = vocab["object_name_to_idx"]["__image__"]
    flat = [(f, b) for f in facts for b in range(len(f["ids"]))]
    assert [r["image_id"] for r in rows] == [f["ids"][b] for f, b in flat]
    for r, (f, b) in zip(rows, flat):
        keep = f["counted"][b] if "counted" in f else (f["boxes"][b] != -1).any(-1) & (f["objs"][b, :, 0] != image_id)
        assert int(keep.sum()) > 0 and not bool(keep[-1])                          # the __image__ row is never counted
        assert r["objects"] == authored.object_names(f["objs"][b][keep].tolist(), vocab)
        assert torch.equal(_bits(r["gt_boxes"]), f["boxes"][b][keep].reshape(-1).view(torch.int32))
        if "boxes_pred" in f:
            assert torch.equal(_bits(r["predicted_boxes"]), f["boxes_pred"][b][keep].reshape(-1).view(torch.int32))
            assert torch.equal(_bits(r["iou"]), f["iou"][b][keep].view(torch.int32))
        else:
            assert "predicted_boxes" not in r and "iou" not in r


def _walk(cuda, root, out, extra, deprocess, **kw):
    """One dataset folder through generate_split and through the calls it is made of."""
    from canonicalsg2im_amd.sample import Sampler
    from canonicalsg2im_amd.split import generate_split
    ds, opt = _opt(root, extra)
    trainer, ckpt = _checkpoint(opt, cuda)
    sampler = Sampler(opt, cuda, ckpt)
    metrics, rows = generate_split(sampler, _batches(ds, opt, sampler, cuda), out, deprocess=deprocess, draw_boxes=True,
                                   split="val", **kw)
    pics, facts, totals = _expected(Sampler(opt, cuda, ckpt), _batches(ds, opt, sampler, cuda), deprocess, cuda)
    return {"ds": ds, "opt": opt, "trainer": trainer, "ckpt": ckpt, "sampler": sampler, "metrics": metrics, "rows": rows,
            "pics": pics, "facts": facts, "totals": totals, "out": out, "deprocess": deprocess}


@pytest.fixture(scope="module")
def coco(cuda, tmp_path_factory):
    """The `coco` val folder of five pictures, walked once with three writer threads; shared, left unchanged."""
    root = str(tmp_path_factory.mktemp("splitroot"))
    pc.write_folder(root, split="val")
    run = _walk(cuda, root, str(tmp_path_factory.mktemp("split_coco")), [], "imagenet", num_writers=3)
    run["root"] = root
    return run


@pytest.mark.timeout(300)
def test_coco_val_folder_every_file_equals_the_existing_calls(coco):
    ids = _check_files(coco["out"], coco["pics"], coco["facts"], ALL_SETS)
    assert ids == [11, 12, 13, 14, 15] and [len(f["ids"]) for f in coco["facts"]] == [2, 2, 1]
    s = coco["sampler"]
    print("split walk: %d replayed, %d eager calls" % (s.replays, s.eager_calls))
    assert s.replays > 0 and s.eager_calls > 0
    for p in coco["pics"]:                                                          # outlines only in layout/
        assert not torch.equal(p["layout/gt"], p["gt"]) and not torch.equal(p["layout/pred"], p["generation/pred_box_pred_mask"])


@pytest.mark.timeout(300)
def test_rows_layouts_json_and_metrics(coco, cuda):
    from canonicalsg2im_amd.evaluate import Evaluator
    vocab = coco["opt"].vocab
    _check_rows(coco["rows"], coco["facts"], vocab)
    doc = json.loads(open(os.path.join(coco["out"], "layouts.json")).read())
    assert {k: doc[k] for k in ("dataset", "split", "image_size", "deprocess", "rescale")} == \
        {"dataset": "coco", "split": "val", "image_size": [64, 64], "deprocess": "imagenet", "rescale": True}
    assert doc["images"] == coco["rows"] and doc["metrics"] == coco["metrics"]
    _check_rows(doc["images"], coco["facts"], vocab)
    assert all(isinstance(o, str) for r in doc["images"] for o in r["objects"])    # one attribute: names
    t, m = coco["totals"], coco["metrics"]
    assert m == {"avg_iou": float(t[0] / t[3]), "total_iou_05": float(t[1] / t[3]), "total_iou_03": float(t[2] / t[3]),
                 "num_boxes": float(t[3])}
    assert m["num_boxes"] == sum(len(r["objects"]) for r in coco["rows"]) > 0 and m["avg_iou"] > 0
    tr = coco["trainer"]
    losses, _, table = Evaluator(tr).check_model(_batches(coco["ds"], coco["opt"], tr, cuda), use_gt=False)
    print("metrics: %s; check_model: %s" % (m, {k: float(losses[k]) for k in ("avg_iou", "total_iou_05", "total_iou_03")}))
    for k in ("avg_iou", "total_iou_05", "total_iou_03"):
        assert losses[k].dtype == torch.float64 and float(losses[k]) == m[k], k
    assert table["image_id"].tolist() == [r["image_id"] for r in coco["rows"]]


@pytest.mark.timeout(300)
def test_one_writer_thread_and_a_cut_run_write_the_same_files(coco, cuda, tmp_path):
    from canonicalsg2im_amd.split import generate_split
    out = str(tmp_path / "one")
    s = coco["sampler"]
    metrics, rows = generate_split(s, _batches(coco["ds"], coco["opt"], s, cuda), out, deprocess="imagenet", draw_boxes=True,
                                   split="val", num_writers=1)
    assert metrics == coco["metrics"] and rows == coco["rows"]
    _check_files(out, coco["pics"], coco["facts"], ALL_SETS)
    # --max_pictures 3 cuts the second batch; no outlines asked for, no layout/; jpg where asked
    cut = str(tmp_path / "cut")
    metrics3, rows3 = generate_split(s, _batches(coco["ds"], coco["opt"], s, cuda), cut, deprocess="imagenet", max_pictures=3,
                                     image_format="jpg", num_writers=2)
    assert rows3 == coco["rows"][:3] and metrics3["num_boxes"] == sum(len(r["objects"]) for r in rows3)
    assert sorted(os.listdir(cut)) == ["generation", "gt", "layouts.json"]
    assert sorted(os.listdir(os.path.join(cut, "gt"))) == ["11.jpg", "12.jpg", "13.jpg"]
    # without out_dir: the same rows and figures, nothing written
    metrics0, rows0 = generate_split(s, _batches(coco["ds"], coco["opt"], s, cuda), deprocess="imagenet")
    assert metrics0 == coco["metrics"] and rows0 == coco["rows"]
    with pytest.raises(ValueError, match="'imagenet' or 'decode_img'.*'srgb'"):
        generate_split(s, [], deprocess="srgb")


@pytest.mark.timeout(300)
def test_a_graph_captured_with_one_deprocess_is_not_replayed_for_the_other(coco, cuda):
    from canonicalsg2im_amd.sample import Sampler
    s = Sampler(coco["opt"], cuda, coco["ckpt"])
    batches = _batches(coco["ds"], coco["opt"], s, cuda)
    imgs, objs, boxes, trip, _, tt, masks, _ = next(batches)
    batches.close()
    a = [s.generate(objs, trip, tt, boxes_gt=boxes, deprocess="imagenet")[0] for _ in range(3)]
    b = [s.generate(objs, trip, tt, boxes_gt=boxes, deprocess="decode_img")[0] for _ in range(3)]
    assert s.replays == 4 and s.eager_calls == 2, (s.replays, s.eager_calls)
    assert torch.equal(a[0], a[2]) and torch.equal(b[0], b[2]) and not torch.equal(a[2], b[2])
    assert torch.equal(a[0], s.generate(objs, trip, tt, boxes_gt=boxes)[0])         # the default is imagenet
    with pytest.raises(ValueError, match="'imagenet' or 'decode_img'"):
        s.generate(objs, trip, tt, deprocess="srgb")


# --------------------------------------------------------------------------------------------- 3. the other folders
@pytest.mark.timeout(300)
def test_packed_clevr_folder_four_attribute_objects_through_decode_img(cuda, tmp_path):
    root = str(tmp_path / "root")
    cc.write_folder(root, split="val")
    run = _walk(cuda, root, str(tmp_path / "out"), ["--dataset", "packed_clevr"], "decode_img", num_writers=2)
    assert _check_files(run["out"], run["pics"], run["facts"], ALL_SETS) == [10, 11, 12, 13, 14]
    _check_rows(run["rows"], run["facts"], run["opt"].vocab)
    assert [len(r["objects"]) for r in run["rows"]] == cc.FOLDER_COUNTS
    first = cc.folder_scene(0, "val")["objects"][0]
    assert run["rows"][0]["objects"][0] == {a: first[a] for a in ("shape", "color", "material", "size")}
    assert json.load(open(os.path.join(run["out"], "layouts.json")))["deprocess"] == "decode_img"
    assert run["sampler"].replays > 0


@pytest.mark.timeout(300)
def test_packed_vg_folder_with_objects_drawn_from_a_seeded_stream(cuda, tmp_path):
    root = str(tmp_path / "root")
    vc.write_folder(root, split="val")
    run = _walk(cuda, root, str(tmp_path / "out"), ["--dataset", "packed_vg"], "decode_img", num_writers=2)
    assert _check_files(run["out"], run["pics"], run["facts"], ALL_SETS) == vc.golden()[0]["image_ids"] == [100, 101, 2317, 7]
    _check_rows(run["rows"], run["facts"], run["opt"].vocab)
    assert run["sampler"].replays > 0


@pytest.mark.timeout(300)
def test_packed_coco_reads_the_coco_folder(coco, cuda, tmp_path):
    run = _walk(cuda, coco["root"], str(tmp_path / "out"), ["--dataset", "packed_coco"], "imagenet", num_writers=2)
    assert _check_files(run["out"], run["pics"], run["facts"], ALL_SETS) == [11, 12, 13, 14, 15]
    _check_rows(run["rows"], run["facts"], run["opt"].vocab)
    assert [r["gt_boxes"] for r in run["rows"]] == [r["gt_boxes"] for r in coco["rows"]]      # the same annotations
    for p, q in zip(run["pics"], coco["pics"]):
        assert torch.equal(p["gt"], q["gt"])                                        # and the same pictures


# --------------------------------------------------------------------------------------------- 4. layouts
@pytest.mark.timeout(300)
def test_layouts_round_trip_without_the_graph_part(coco, cuda, tmp_path):
    from canonicalsg2im_amd.sample import Sampler
    from canonicalsg2im_amd.split import generate_layouts
    rows = json.load(open(os.path.join(coco["out"], "layouts.json")))["images"]
    s = Sampler(coco["opt"], cuda, coco["ckpt"])

    def boom(*a, **k):
        raise AssertionError("the scene-graph encoder was run for a layout")

    s.model.sg_to_layout.forward = boom
    with pytest.raises(AssertionError, match="encoder was run"):
        s.model.sg_to_layout(None, None, None, None)
    for which in ("pred", "gt"):
        out = str(tmp_path / which)
        assert generate_layouts(s, rows, which, out, deprocess="imagenet", batch_size=2, num_writers=2) == 5
        name = "generation/%s_box_%s_mask" % (which, which)
        assert sorted(os.listdir(os.path.join(out, "generation"))) == ["%s_box_%s_mask" % (which, which)]
        for r in rows:
            got = _decoded(os.path.join(out, name, "%d.png" % r["image_id"]))
            want = _decoded(os.path.join(coco["out"], name, "%d.png" % r["image_id"]))
            assert torch.equal(got, want), "%s/%d.png: %d bytes differ" % (name, r["image_id"], int((got != want).sum()))
    held = generate_layouts(s, rows[:3], "gt", deprocess="imagenet", batch_size=2)   # no out_dir: the pictures themselves
    assert held.dtype == torch.uint8 and tuple(held.shape) == (3, 3, 64, 64)
    assert torch.equal(held, torch.cat([p["generation/gt_box_gt_mask"] for p in coco["pics"]])[:3])
    assert s.replays > 0
    with pytest.raises(ValueError, match="pass boxes_gt"):
        s.generate(torch.zeros((1, 2, 1), dtype=torch.int64, device=cuda), None, None)


# --------------------------------------------------------------------------------------------- 5. no graph part; errors
@pytest.mark.timeout(300)
def test_a_model_without_the_graph_part_writes_no_pred_folder(coco, cuda, tmp_path):
    from canonicalsg2im_amd.sample import Sampler
    from canonicalsg2im_amd.split import generate_split
    ds, opt = _opt(coco["root"], ["--skip_graph_model", "1"])
    torch.manual_seed(6)
    s = Sampler(opt, cuda)
    assert not s.model.has_graph
    out = str(tmp_path / "out")
    metrics, rows = generate_split(s, _batches(ds, opt, s, cuda), out, deprocess="imagenet", draw_boxes=True, num_writers=2)
    pics, facts, _ = _expected(Sampler(opt, cuda, model=s.model), _batches(ds, opt, s, cuda), "imagenet", cuda)
    _check_files(out, pics, facts, ["gt", "generation/gt_box_gt_mask", "layout/gt"])
    _check_rows(rows, facts, opt.vocab)
    assert metrics == {} and not os.path.exists(os.path.join(out, "generation", "pred_box_pred_mask"))
    assert [r["gt_boxes"] for r in rows] == [r["gt_boxes"] for r in coco["rows"]]


def _counted(batches, seen):
    for b in batches:
        seen.append(b[7].cpu().tolist())
        yield b


@pytest.mark.timeout(300)
def test_a_writer_error_stops_the_run(coco, cuda, tmp_path):
    from canonicalsg2im_amd.split import generate_split
    s = coco["sampler"]
    # out_dir/gt is a regular file: the first batch's files cannot be written
    out = tmp_path / "out"
    out.mkdir()
    (out / "gt").write_text("a file where a directory is expected")
    seen = []
    with pytest.raises(OSError):
        generate_split(s, _counted(_batches(coco["ds"], coco["opt"], s, cuda), seen), str(out), deprocess="imagenet", num_writers=2)
    print("gt is a file: raised after batches %s" % seen)
    assert len(seen) <= 2 and (out / "gt").is_file() and not (out / "layouts.json").exists()
    # one file's name is taken by a directory: a writer THREAD fails, while later batches are walked.  Batches of one
    # picture: the files of batch 0 are handed to the threads while batch 1 is walked, so the error is seen before batch 3
    out = tmp_path / "late"
    (out / "gt" / "11.png").mkdir(parents=True)
    seen = []
    before = s.replays + s.eager_calls
    with pytest.raises(IsADirectoryError):
        generate_split(s, _counted(_batches(coco["ds"], coco["opt"], s, cuda, batch_size=1), seen), str(out), deprocess="imagenet",
                       num_writers=2)
    print("11.png is a directory: raised after batches %s, %d generate calls" % (seen, s.replays + s.eager_calls - before))
    assert seen[0] == [11] and len(seen) <= 3 and s.replays + s.eager_calls - before <= 6
    written = {n for d, _, names in os.walk(out) for n in names}
    assert not written & {"14.png", "15.png", "layouts.json"}, written
    import threading
    assert not [t for t in threading.enumerate() if t.name.startswith("csg-file-writer")]
    # a dataset that repeats an image id: refused when the second one comes, the first one's files are there
    out = tmp_path / "twice"
    batches = _batches(coco["ds"], coco["opt"], s, cuda)
    first = next(batches)
    batches.close()
    with pytest.raises(ValueError, match="image id 11 a second time"):
        generate_split(s, [first, first], str(out), deprocess="imagenet", num_writers=2)
    assert sorted(os.listdir(out / "gt")) == ["11.png", "12.png"]


# --------------------------------------------------------------------------------------------- 6. the command lines
@pytest.mark.timeout(600)
def test_command_lines_sample_a_split_and_its_layouts(coco, cuda, tmp_path, capsys):
    from canonicalsg2im_amd.scripts import sample as cli, train as train_cli
    root = coco["root"]
    image_dir, _ = pc.write_folder(root)                                            # the train split, beside val
    ck_dir = str(tmp_path / "ck")
    common = [a for a in MODEL] + ["--dataroot", root]
    train_cli.main(common + ["--num_iterations", "2", "--print_every", "1", "--output_dir", ck_dir, "--checkpoint_every", "2"])
    capsys.readouterr()
    ck = os.path.join(ck_dir, "itr_2.pt")
    out = str(tmp_path / "pictures")
    cli.main(common + ["--batch_size", "2", "--split", "val", "--checkpoint_name", ck, "--output_dir", out,
                       "--img_deprocess", "imagenet", "--num_writers", "2"])
    lines = capsys.readouterr().out.splitlines()
    assert "data: 5 pictures of %s" % image_dir.replace("train2017", "val2017") in lines, lines
    assert sum(bool(re.fullmatch(r"Iter: 2, SPLIT val avg_iou: [\d.]+ total_iou_03: [\d.]+ total_iou_05: [\d.]+  num_boxes [\d.]+", l))
               for l in lines) == 1, lines
    assert re.fullmatch(r"5 images in [\d.]+ s  \[[\d.]+ img/s\]  \(\d+ replayed, \d+ eager calls\)", lines[-1]), lines
    for s in ALL_SETS:
        assert sorted(os.listdir(os.path.join(out, s))) == ["%d.png" % i for i in range(11, 16)], s
    doc = json.load(open(os.path.join(out, "layouts.json")))
    assert doc["split"] == "val" and doc["deprocess"] == "imagenet" and len(doc["images"]) == 5
    # --draw_boxes 0 and a cap
    bare = str(tmp_path / "bare")
    cli.main(common + ["--batch_size", "2", "--split", "train", "--checkpoint_name", ck, "--output_dir", bare, "--draw_boxes", "0",
                       "--max_pictures", "3"])
    assert "data: 5 pictures of %s" % image_dir in capsys.readouterr().out.splitlines()
    assert sorted(os.listdir(bare)) == ["generation", "gt", "layouts.json"] and len(os.listdir(os.path.join(bare, "gt"))) == 3
    assert json.load(open(os.path.join(bare, "layouts.json")))["deprocess"] == "decode_img"
    # the layouts of the first run, drawn by the generator alone: the files of that run
    again = str(tmp_path / "again")
    for which in ("pred", "gt"):
        cli.main(common + ["--batch_size", "2", "--layouts", os.path.join(out, "layouts.json"), "--layout_boxes", which,
                           "--checkpoint_name", ck, "--output_dir", again, "--img_deprocess", "imagenet"])
        line = capsys.readouterr().out.strip().splitlines()[-1]
        assert re.fullmatch(r"5 images in [\d.]+ s  \[[\d.]+ img/s\]  \(\d+ replayed, \d+ eager calls\)", line), line
        name = os.path.join("generation", "%s_box_%s_mask" % (which, which))
        for i in range(11, 16):
            assert torch.equal(_decoded(os.path.join(again, name, "%d.png" % i)), _decoded(os.path.join(out, name, "%d.png" % i)))
    bad = tmp_path / "bad.json"
    bad.write_text(json.dumps({"images": doc["images"][:1] + [dict(doc["images"][1], objects=["zebra"])]}))
    with pytest.raises(SystemExit, match="layouts row 1: .*'zebra'"):
        cli.main(common + ["--layouts", str(bad), "--checkpoint_name", ck, "--output_dir", again])
    # a checkpoint of another vocabulary is refused on the host
    other = dict(torch.load(ck, map_location="cpu"))
    other["vocab"] = dict(other["vocab"], pred_idx_to_name=other["vocab"]["pred_idx_to_name"] + ["one more"])
    torch.save(other, tmp_path / "other.pt")
    with pytest.raises(SystemExit, match="the val split's predicates"):
        cli.main(common + ["--split", "val", "--checkpoint_name", str(tmp_path / "other.pt")])
    # and the invocation without --split writes what it wrote before
    plain = tmp_path / "plain"
    cli.main(MODEL[:-2] + ["--batch_size", "2", "--num_samples", "2", "--output_dir", str(plain)])
    line = capsys.readouterr().out.strip().splitlines()[-1]
    assert re.fullmatch(r"2 images in [\d.]+ s  \[[\d.]+ img/s\]  \(\d+ replayed, \d+ eager calls\)", line), line
    assert sorted(p.name for p in plain.iterdir()) == ["img_000000.png", "img_000001.png"]
