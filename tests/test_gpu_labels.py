"""The boxes' names on the layout pictures, on a real MI355X: the label kernel (csg_draw_labels_u8, csrc/overlay.hip)
against its numpy restatement (tests/label_cases.py) byte for byte, and the three places that call it
(`Sampler.generate_from_graphs(labels=True)`, `split.generate_split(draw_labels=True)`, `scripts.sample --draw_labels 1`)
against `ops.draw_labels_u8(ops.draw_boxes_u8(...))` composed by hand from what they return or write.

No tolerance anywhere: every comparison is of bytes.  Shapes: the table's 24 x 40 and 16 x 16 pictures; seeded random
weights at 64 x 64 as tests/test_gpu_authored.py builds them, four authored graphs, two synthetic batches of two."""
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import label_cases as lc
import overlay_cases as oc
from conftest import load_golden
from test_authored_graphs import fixture_vocab

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TINY = ["--image_size", "64,64", "--ngf", "4", "--ndf", "8", "--gconv_dim", "32", "--gconv_hidden_dim", "64",
        "--gconv_num_layers", "2", "--embedding_dim", "8", "--no_vgg_loss", "--batch_size", "4"]
FOUR = (0, 1, 3, 4)            # the sparse and the dense graph of three and of four objects
BOX_BIAS = [0.2, 0.25, 0.45, 0.4]          # the untrained box head's last bias: boxes with an area (test_gpu_authored.py)
CASES = lc.table()


@pytest.fixture(scope="module")
def cuda():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device("cuda:0")


def _on(cuda, case):
    return [torch.from_numpy(case[k]).to(cuda) for k in ("img", "boxes", "objs", "palette")]


# --------------------------------------------------------------------------------------------- 1. the label kernel
@pytest.mark.timeout(120)
@pytest.mark.parametrize("ci", range(len(CASES)), ids=[c["name"] for c in CASES])
def test_draw_labels_u8_equals_the_restatement_byte_for_byte(cuda, ci):
    from canonicalsg2im_amd import ops
    from canonicalsg2im_amd.font5x7 import FONT
    c = CASES[ci]
    want = lc.expected(c, FONT)
    img, boxes, objs, pal = _on(cuda, c)
    kept = img.clone()
    got = ops.draw_labels_u8(img, boxes, objs, c["image_id"], pal, c["labels"])
    again = ops.draw_labels_u8(img, boxes, objs, c["image_id"], pal, c["labels"], font=torch.from_numpy(FONT.copy()).to(cuda))
    torch.cuda.synchronize()
    assert got.dtype == torch.uint8 and tuple(got.shape) == tuple(img.shape) and got.data_ptr() != img.data_ptr()
    differing = int((got.cpu().numpy() != want).sum())
    print("draw_labels_u8 %s: %d differing bytes of %d, %d painted, %d ink" % (
        c["name"], differing, want.size, int((want != c["img"]).sum()), int((want == 0).all(1).sum())))
    assert differing == 0, c["name"]
    assert torch.equal(img, kept), "the input picture was written"
    assert torch.equal(got, again), "a second call differs"


@pytest.mark.timeout(120)
def test_draw_labels_u8_refuses_what_it_cannot_draw(cuda):
    from canonicalsg2im_amd import ops
    c = CASES[0]
    img, boxes, objs, pal = _on(cuda, c)
    labels = c["labels"]
    with pytest.raises(RuntimeError, match="multiple of 4"):
        ops.draw_labels_u8(img[..., :15], boxes, objs, 0, pal, labels)
    with pytest.raises(RuntimeError, match="uint8"):
        ops.draw_labels_u8(img.float(), boxes, objs, 0, pal, labels)
    with pytest.raises(RuntimeError, match="int64"):
        ops.draw_labels_u8(img, boxes, objs.int(), 0, pal, labels)
    with pytest.raises(RuntimeError, match=r"boxes \(B,O,4\)"):
        ops.draw_labels_u8(img, boxes[:, :4], objs, 0, pal, labels)
    with pytest.raises(RuntimeError, match="2 sequences of 5"):
        ops.draw_labels_u8(img, boxes, objs, 0, pal, labels[:1])
    with pytest.raises(RuntimeError, match="2 sequences of 5"):
        ops.draw_labels_u8(img, boxes, objs, 0, pal, [row[:4] for row in labels])
    with pytest.raises(RuntimeError, match="str or None"):
        ops.draw_labels_u8(img, boxes, objs, 0, pal, [[1, 2, 3, 4, 5]] * 2)
    with pytest.raises(RuntimeError, match=r"font must be uint8 \(95, 7\)"):
        ops.draw_labels_u8(img, boxes, objs, 0, pal, labels, font=torch.zeros((95, 8), dtype=torch.uint8, device=cuda))
    with pytest.raises(RuntimeError, match="at most 256 rows"):
        ops.draw_labels_u8(img, boxes[:, :1].expand(2, 257, 4), objs[:, :1].expand(2, 257, 2), 0, pal, [["a"] * 257] * 2)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.draw_labels_u8(img.cpu(), boxes.cpu(), objs.cpu(), 0, pal.cpu(), labels)


# --------------------------------------------------------------------------------------------- 2. authored graphs
@pytest.fixture(scope="module")
def fx():
    meta, arrays = load_golden("authored_graphs")
    return meta, fixture_vocab(meta)


def _checkpoint(opt, cuda, vocab, seed=5):
    """Fresh seeded weights with the box head's last bias set to a box inside the frame (test_gpu_authored.py)."""
    from canonicalsg2im_amd.sample import Sampler
    torch.manual_seed(seed)
    fresh = Sampler(opt, cuda)
    ckpt = {"model_state": {k: v.detach().cpu().clone() for k, v in fresh.model.state_dict().items()}, "vocab": vocab}
    last = sorted((k for k in ckpt["model_state"] if re.search(r"box_net\.\d+\.bias$", k)),
                  key=lambda k: int(re.search(r"box_net\.(\d+)\.", k).group(1)))[-1]
    assert tuple(ckpt["model_state"][last].shape) == (4,)
    ckpt["model_state"][last] = torch.tensor(BOX_BIAS)
    return ckpt


@pytest.fixture(scope="module")
def drawn(cuda, fx, tmp_path_factory):
    """Three calls with labels (eager, capturing, replayed) on one sampler and four without on another, alternately with
    and without the argument.  Computed once, shared, left unchanged."""
    from canonicalsg2im_amd import train as T
    from canonicalsg2im_amd.sample import Sampler
    meta, vocab = fx
    opt = T.make_opt(vocab, TINY)
    ckpt = _checkpoint(opt, cuda, vocab)
    path = tmp_path_factory.mktemp("labels") / "fresh.pt"
    torch.save(ckpt, path)
    graphs = [meta["graphs"][g] for g in FOUR]
    s = Sampler(opt, cuda, ckpt)
    labelled = [s.generate_from_graphs(graphs, overlay=True, labels=True) for _ in range(3)]
    assert (s.eager_calls, s.replays) == (1, 2), (s.eager_calls, s.replays)
    p = Sampler(opt, cuda, ckpt)
    plain = [p.generate_from_graphs(graphs, overlay=True, **kw) for kw in ({}, {"labels": False}, {}, {"labels": False})]
    assert (p.eager_calls, p.replays) == (1, 3), (p.eager_calls, p.replays)
    torch.cuda.synchronize()
    return {"opt": opt, "ckpt": ckpt, "path": str(path), "graphs": graphs, "labelled": labelled, "plain": plain, "sampler": s}


def _compose(cuda, vocab, graphs, imgs, boxes):
    """draw_labels_u8(draw_boxes_u8(...)) by hand: the encoded objects, the default palette, thickness 2."""
    from canonicalsg2im_amd import authored, ops
    objs = authored.encode_graphs(graphs, vocab)[0].to(cuda)
    pal = torch.tensor(authored.DEFAULT_PALETTE, dtype=torch.uint8).to(cuda)
    image_id = vocab["object_name_to_idx"]["__image__"]
    outlined = ops.draw_boxes_u8(imgs, boxes.float(), objs, image_id, pal, 2)
    return outlined, ops.draw_labels_u8(outlined, boxes.float(), objs, image_id, pal, authored.object_labels(graphs))


@pytest.mark.timeout(300)
def test_generate_from_graphs_with_labels_equals_the_hand_composition_eager_and_replayed(cuda, fx, drawn):
    from canonicalsg2im_amd import authored
    from canonicalsg2im_amd.font5x7 import FONT
    _, vocab = fx
    for k, (imgs, boxes, overlays) in enumerate(drawn["labelled"]):
        outlined, want = _compose(cuda, vocab, drawn["graphs"], imgs, boxes)
        assert overlays.dtype == torch.uint8 and tuple(overlays.shape) == (4, 3, 64, 64)
        assert torch.equal(overlays, want), "call %d: %d bytes differ" % (k, int((overlays != want).sum()))
        assert not torch.equal(overlays, outlined), "no label was drawn: the comparison would hold for any label kernel"
    first = drawn["labelled"][0]
    for k, run in enumerate(drawn["labelled"][1:], 1):
        assert all(torch.equal(a, b) for a, b in zip(run, first)), "call %d differs from the eager call" % k
    # and the whole picture once on the host: outlines, then names, by the two restatements
    imgs, boxes, overlays = (t.cpu().numpy() for t in first)
    objs = authored.encode_graphs(drawn["graphs"], vocab)[0].numpy()
    pal = np.asarray(authored.DEFAULT_PALETTE, np.uint8)
    labels = authored.object_labels(drawn["graphs"])
    assert labels[0][0] == ", ".join(drawn["graphs"][0]["objects"][0].values()) and labels[0][-1] is None
    host = lc.draw_labels(oc.draw_boxes(imgs, boxes, objs, 0, pal, 2), boxes, objs, 0, pal, labels, FONT)
    print("labelled overlays: %d bytes differ from the host's, %d from the pictures" % (
        int((overlays != host).sum()), int((overlays != imgs).sum())))
    assert np.array_equal(overlays, host)
    with pytest.raises(ValueError, match="overlay=True"):
        drawn["sampler"].generate_from_graphs(drawn["graphs"], labels=True)


@pytest.mark.timeout(300)
def test_labels_false_is_byte_identical_to_not_passing_the_argument(cuda, fx, drawn):
    _, vocab = fx
    first = drawn["plain"][0]                                            # eager, without the argument
    for k, run in enumerate(drawn["plain"][1:], 1):                      # labels=False capturing; both replayed
        assert all(torch.equal(a.view(torch.uint8), b.view(torch.uint8)) for a, b in zip(run, first)), "call %d" % k
    # the outlined pictures are the first half of the hand composition, and the labelled runs drew on the same pictures
    outlined, _ = _compose(cuda, vocab, drawn["graphs"], first[0], first[1])
    assert torch.equal(first[2], outlined)
    assert torch.equal(drawn["labelled"][0][0], first[0]) and torch.equal(drawn["labelled"][0][1], first[1])
    assert not torch.equal(drawn["labelled"][0][2], first[2])


@pytest.mark.timeout(300)
def test_command_line_in_a_fresh_process_writes_the_labelled_layouts(cuda, fx, drawn, tmp_path):
    from PIL import Image
    src = tmp_path / "graphs.json"
    src.write_text(json.dumps(drawn["graphs"]))
    out = tmp_path / "out"
    r = subprocess.run([sys.executable, "-m", "canonicalsg2im_amd.scripts.sample", "--scene_graphs", str(src), "--output_dir",
                        str(out), "--checkpoint_name", drawn["path"], "--draw_labels", "1"] + TINY, cwd=ROOT,
                       env=dict(os.environ, PYTHONPATH=ROOT), capture_output=True, text=True, timeout=280)
    assert r.returncode == 0, r.stderr[-3000:]
    imgs, _, overlays = drawn["labelled"][0]
    assert sorted(p.name for p in out.iterdir()) == sorted(
        ["graphs.json"] + ["img_%06d_%s.png" % (i, k) for i in range(4) for k in ("generated", "layout")])
    for i in range(4):
        for kind, t in (("generated", imgs), ("layout", overlays)):
            png = np.asarray(Image.open(out / ("img_%06d_%s.png" % (i, kind))))
            assert png.dtype == np.uint8 and np.array_equal(png, t[i].permute(1, 2, 0).cpu().numpy()), (i, kind)


# --------------------------------------------------------------------------------------------- 3. a split
def _decoded(path):
    from PIL import Image
    with Image.open(path) as im:
        assert im.mode == "RGB"
        return torch.from_numpy(np.asarray(im).copy()).permute(2, 0, 1)


@pytest.mark.timeout(300)
def test_generate_split_labels_the_two_layout_sets_and_nothing_else(cuda, tmp_path):
    from canonicalsg2im_amd import authored, ops, train as T
    from canonicalsg2im_amd.sample import Sampler
    from canonicalsg2im_amd.sg2im.data.loader import HostBatch
    from canonicalsg2im_amd.split import SETS, generate_split
    from canonicalsg2im_amd.synth import BatchConfig, make_batch, make_vocab
    vocab = make_vocab("tiny")
    opt = T.make_opt(vocab, TINY[:-1] + ["2"])
    sampler = Sampler(opt, cuda, _checkpoint(opt, cuda, vocab))
    host = [list(make_batch(vocab, BatchConfig(2, 64, 2, 5, "packed"), seed=s)) for s in (11, 12)]
    host[1][7] = host[1][7] + 2                                           # image ids 0, 1 and 2, 3

    def batches():
        return [HostBatch([None if t is None else t.to(cuda) for t in b], b[1]) for b in host]

    kw = dict(deprocess="imagenet", draw_boxes=True, num_writers=2)
    plain, named = str(tmp_path / "plain"), str(tmp_path / "named")
    metrics0, rows0 = generate_split(sampler, batches(), plain, **kw)
    metrics1, rows1 = generate_split(sampler, batches(), named, draw_labels=True, **kw)
    assert metrics1 == metrics0 and rows1 == rows0
    assert json.load(open(os.path.join(named, "layouts.json"))) == json.load(open(os.path.join(plain, "layouts.json")))
    pal = torch.tensor(authored.DEFAULT_PALETTE, dtype=torch.uint8).to(cuda)
    image_id = vocab["object_name_to_idx"]["__image__"]
    drawn_labels = 0
    for b in host:
        dev = [None if t is None else t.to(cuda) for t in b]
        labels = authored.labels_from_objs(b[1], vocab)
        assert any(l is not None for row in labels for l in row)
        boxes_pred = sampler.generate(dev[1], dev[3], dev[5])[1]
        ids = b[7].tolist()
        for name in SETS:
            got = torch.stack([_decoded(os.path.join(named, name, "%d.png" % i)) for i in ids])
            was = torch.stack([_decoded(os.path.join(plain, name, "%d.png" % i)) for i in ids])
            if not name.startswith("layout/"):
                assert torch.equal(got, was), name
                continue
            boxes = dev[2] if name == "layout/gt" else boxes_pred
            want = ops.draw_labels_u8(was.to(cuda), boxes.float(), dev[1], image_id, pal, labels).cpu()
            assert torch.equal(got, want), "%s: %d bytes differ" % (name, int((got != want).sum()))
            assert not torch.equal(got, was), "%s: no label was drawn" % name
            drawn_labels += 1
    assert drawn_labels == 4
    # batches that do not carry their ids on the host are refused, and so are names without outlines: nothing is launched
    calls = sampler.eager_calls + sampler.replays
    with pytest.raises(ValueError, match="objs_host"):
        generate_split(sampler, [list(b) for b in batches()], draw_labels=True, **kw)
    with pytest.raises(ValueError, match="draw_boxes=True"):
        generate_split(sampler, batches(), deprocess="imagenet", draw_labels=True)
    assert sampler.eager_calls + sampler.replays == calls


@pytest.mark.timeout(300)
@pytest.mark.parametrize("dataset", ["coco", "packed_clevr", "packed_vg"])
def test_folder_batches_carry_the_ids_of_their_device_objects_on_the_host(cuda, tmp_path, dataset):
    """What generate_split(draw_labels=True) names the boxes from: `objs_host` of a BatchBuilder's batch equals the batch's
    device objects, `__image__` row included (read back here, in the test, only)."""
    import clevr_cases as cc
    import pair_cases as pc
    import vg_cases as vc
    from canonicalsg2im_amd import authored
    from canonicalsg2im_amd.sg2im.data.loader import HostBatch
    from test_gpu_split import _batches, _opt
    root = str(tmp_path / "root")
    {"coco": pc, "packed_clevr": cc, "packed_vg": vc}[dataset].write_folder(root, split="val")
    ds, opt = _opt(root, ["--dataset", dataset])
    seen = 0
    for batch in _batches(ds, opt, None, cuda):
        assert isinstance(batch, HostBatch) and len(batch) == 8 and not batch.objs_host.is_cuda
        assert batch.objs_host.dtype == torch.int64 and torch.equal(batch.objs_host, batch[1].cpu())
        labels = authored.labels_from_objs(batch.objs_host, ds.vocab)
        assert all(row[-1] is None for row in labels) and all(isinstance(row[0], str) for row in labels)
        seen += len(labels)
    assert seen == len(ds)


@pytest.mark.timeout(300)
def test_generate_layouts_writes_labelled_layouts_from_the_rows_names(cuda, tmp_path):
    from canonicalsg2im_amd import authored, ops, train as T
    from canonicalsg2im_amd.sample import Sampler
    from canonicalsg2im_amd.split import generate_layouts, layout_batch, encode_layouts
    from canonicalsg2im_amd.synth import make_vocab
    vocab = make_vocab("tiny")
    opt = T.make_opt(vocab, TINY[:-1] + ["2"])
    sampler = Sampler(opt, cuda, _checkpoint(opt, cuda, vocab))
    rows = [{"image_id": 7, "objects": ["obj_1", "obj_2"], "gt_boxes": [[0.1, 0.1, 0.5, 0.4], [0.4, 0.5, 0.5, 0.4]]},
            {"image_id": 9, "objects": ["obj_3"], "gt_boxes": [[0.2, 0.3, 0.6, 0.6]]}]
    bare = generate_layouts(sampler, rows, "gt", deprocess="imagenet", batch_size=2)
    pics, named = generate_layouts(sampler, rows, "gt", deprocess="imagenet", batch_size=2, draw_labels=True)
    assert torch.equal(pics, bare)
    objs, boxes = (t.to(cuda) for t in layout_batch(encode_layouts(rows, "gt", vocab), vocab))
    pal = torch.tensor(authored.DEFAULT_PALETTE, dtype=torch.uint8).to(cuda)
    want = ops.draw_labels_u8(ops.draw_boxes_u8(pics.to(cuda), boxes, objs, 0, pal, 2), boxes, objs, 0, pal,
                              [["obj_1", "obj_2", None], ["obj_3", None, None]])
    assert torch.equal(named, want.cpu()) and not torch.equal(named, pics)
    out = str(tmp_path / "out")
    assert generate_layouts(sampler, rows, "gt", out, deprocess="imagenet", batch_size=2, draw_labels=True, num_writers=2) == 2
    for i, image_id in enumerate((7, 9)):
        assert torch.equal(_decoded(os.path.join(out, "layout", "gt", "%d.png" % image_id)), named[i])
        assert torch.equal(_decoded(os.path.join(out, "generation", "gt_box_gt_mask", "%d.png" % image_id)), pics[i])
