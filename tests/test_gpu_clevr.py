"""The CLEVR input stage on a real MI355X: csrc/clevr.hip against the reference's recorded boxes, the 4-byte pixels of
csrc/preprocess.hip against the host restatements of tests/clevr_cases.py (which tests/test_clevr_cases.py pins to the
reference, Pillow and torch on the CPU), and the CLEVR folder dataset that feeds both.

No tolerance anywhere: the boxes are + - * / in fp64 and one rounding to fp32, the resize is integer arithmetic on
fp64-derived integer coefficients, the float stage is three correctly rounded fp32 operations; both sides are defined
operation by operation, so the bits are equal."""
import os

import numpy as np
import pytest
import torch

import clevr_cases as cc
import preprocess_cases as pc
from conftest import load_golden

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def cuda():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device("cuda:0")


_REFERENCE = {}


def reference(name, H, W, seed=0):
    """[(source picture, resized uint8 (H,W,3), fp32 (3,H,W))] of a batch of the table: computed once, shared, never
    written to."""
    key = (name, H, W, seed)
    if key not in _REFERENCE:
        out = []
        for img in cc.batch_images(name, seed):
            u8 = pc.pil_resize_u8(cc.rgb_of(img), H, W)
            out.append((img, torch.from_numpy(u8), cc.to_float(u8)))
        _REFERENCE[key] = out
    return _REFERENCE[key]


def run_px(ops, cuda, images, H, W, **kw):
    packed, desc = cc.pack_px(images)
    kw.setdefault("mean", 0.5)
    kw.setdefault("std", 0.5)
    return ops.preprocess_images(torch.from_numpy(packed).to(cuda), torch.from_numpy(desc), H, W, want_u8=True, **kw)


# ------------------------------------------------------------------------------------------------- 1. the boxes
def _golden_on(cuda):
    _, g = load_golden("clevr_boxes")
    objs = torch.zeros(g["shape"].shape + (4,), dtype=torch.int64)
    objs[..., 0] = g["shape"]
    objs[..., 1] = 7                                      # the other attributes are not the kernel's business
    return g, objs, [g["geom"].to(cuda), objs.to(cuda), g["rot"].to(cuda), g["counts"].to(cuda)]


def test_boxes_equal_the_reference_bit_for_bit(cuda):
    from canonicalsg2im_amd import ops
    g, objs, dev = _golden_on(cuda)
    got = ops.clevr_boxes(*dev, objs_host=objs, counts_host=g["counts"])
    read_back = ops.clevr_boxes(*dev)                      # the host copies fetched by the call itself
    one = ops.clevr_boxes(dev[0], dev[1][..., :1].contiguous(), dev[2], dev[3])         # A = 1: the shape ids alone
    torch.cuda.synchronize()
    want = g["boxes"]
    assert got.dtype == torch.float32 and tuple(got.shape) == tuple(want.shape) == (22, 10, 4) and got.is_contiguous()
    differing = int((got.cpu().view(torch.int32) != want.view(torch.int32)).any(-1).sum())
    print("clevr_boxes: %d of %d rows differ from the reference's bits" % (differing, 220))
    assert differing == 0
    assert torch.equal(got.cpu(), want) and torch.equal(read_back, got) and torch.equal(one, got)
    real = torch.arange(10)[None] < g["counts"][:, None]
    assert int(real.sum()) == 183 and bool((got.cpu()[~real] == -1).all()) and bool((got.cpu()[real][:, 2:] > 0).all())
    assert torch.equal(got.cpu(), torch.from_numpy(cc.boxes_fp64(g["geom"].numpy(), g["shape"].numpy(), g["rot"].numpy(),
                                                                 g["counts"].numpy())))


def test_box_refusals_carry_a_message_and_launch_nothing(cuda):
    from canonicalsg2im_amd import _lib, ops
    g, objs, dev = _golden_on(cuda)
    _lib.prof_enable(1)
    _lib.prof_reset()
    try:
        for bad_id in (0, 4, -1):
            bad = objs.clone()
            bad[3, 2, 0] = bad_id
            with pytest.raises(RuntimeError, match="object 2 of scene 3 has shape id %d, 1 .cube. .. 3 .cylinder." % bad_id):
                ops.clevr_boxes(dev[0], bad.to(cuda), dev[2], dev[3], objs_host=bad, counts_host=g["counts"])
        bad = objs.clone()
        bad[0, 5, 0] = 9                                   # scene 0 has one object: row 5 is padding, its id is not looked at
        ops_ok = ops.clevr_boxes(dev[0], bad.to(cuda), dev[2], dev[3], objs_host=bad, counts_host=g["counts"])
        counts = g["counts"].clone()
        counts[1] = 11
        with pytest.raises(RuntimeError, match="scene 1 has 11 objects, 0 .. O = 10"):
            ops.clevr_boxes(dev[0], dev[1], dev[2], counts.to(cuda), objs_host=objs, counts_host=counts)
        O = 1025
        with pytest.raises(RuntimeError, match="bad shape B=1 O=1025"):
            ops.clevr_boxes(torch.zeros(1, O, 5, dtype=torch.float64, device=cuda),
                            torch.ones(1, O, 1, dtype=torch.int64, device=cuda),
                            torch.zeros(1, 2, dtype=torch.float64, device=cuda), torch.zeros(1, dtype=torch.int64, device=cuda))
        B = 65536
        with pytest.raises(RuntimeError, match="bad shape B=65536 O=1 "):
            ops.clevr_boxes(torch.zeros(B, 1, 5, dtype=torch.float64, device=cuda),
                            torch.ones(B, 1, 1, dtype=torch.int64, device=cuda),
                            torch.zeros(B, 2, dtype=torch.float64, device=cuda), torch.zeros(B, dtype=torch.int64, device=cuda))
        with pytest.raises(RuntimeError, match="no CPU path"):
            ops.clevr_boxes(g["geom"], dev[1], dev[2], dev[3])
        with pytest.raises(RuntimeError, match="geom must be contiguous torch.float64"):
            ops.clevr_boxes(dev[0].float(), dev[1], dev[2], dev[3])
        torch.cuda.synchronize()
        assert _lib.prof_read()["clevr_boxes"][1] == 1      # the padding-row call above, and only it
        assert torch.equal(ops_ok.cpu(), g["boxes"])
    finally:
        _lib.prof_enable(0)
        _lib.prof_reset()


def test_a_stale_device_row_becomes_a_padding_row(cuda):
    """The host copies pass, the device buffer disagrees (as under a replayed graph whose buffer was not refreshed): the row
    with the impossible shape id and the rows beyond an impossible count are -1; nothing else changes."""
    from canonicalsg2im_amd import ops
    g, objs, dev = _golden_on(cuda)
    stale = dev[1].clone()
    stale[4, 1, 0] = 5
    counts = dev[3].clone()
    counts[6] = 1000
    counts[7] = -3
    got = ops.clevr_boxes(dev[0], stale, dev[2], counts, objs_host=objs, counts_host=g["counts"]).cpu()
    want = g["boxes"].clone()
    want[4, 1] = -1
    want[7] = -1
    n6 = int(g["counts"][6])
    assert torch.equal(got[:6], want[:6]) and torch.equal(got[7:], want[7:]) and torch.equal(got[6, :n6], want[6, :n6])


# ------------------------------------------------------------------------------------------- 2. 4-byte pixels
@pytest.mark.parametrize("case", cc.CASES, ids=cc.batch_id)
def test_px_batches_equal_pillow_bytes_and_torch_bits(cuda, case):
    from canonicalsg2im_amd import ops
    name, (H, W) = case
    refs = reference(name, H, W)
    f32, u8 = run_px(ops, cuda, [r[0] for r in refs], H, W)
    plain, _ = run_px(ops, cuda, [r[0] for r in refs], H, W, normalize=False)
    torch.cuda.synchronize()
    assert f32.dtype == torch.float32 and tuple(f32.shape) == (len(refs), 3, H, W) and f32.is_contiguous()
    assert u8.dtype == torch.uint8 and tuple(u8.shape) == (len(refs), H, W, 3)
    for i, (img, want_u8, want_f32) in enumerate(refs):
        nb, nf = int((u8[i].cpu() != want_u8).sum()), int((f32[i].cpu() != want_f32).sum())
        print("%s picture %d %s: %d differing bytes, %d differing floats" % (cc.batch_id(case), i, img.shape, nb, nf))
        assert nb == 0 and nf == 0
        assert torch.equal(f32[i].cpu(), want_f32)
        assert torch.equal(plain[i].cpu(), cc.to_float(want_u8.numpy(), normalize=False))


@pytest.mark.parametrize("HW", cc.OUTPUTS, ids=lambda hw: "%dx%d" % hw)
def test_three_byte_batch_gives_the_same_bits_through_either_entry(cuda, HW):
    """The pictures of the mixed batch as RGB, through the three-column call (csg_preprocess, as before this entry existed),
    through the four-column call with 3 bytes per pixel everywhere, and through the four-column call as they are."""
    from canonicalsg2im_amd import ops
    H, W = HW
    refs = reference("mixed", H, W)
    rgb = [cc.rgb_of(r[0]) for r in refs]
    packed, desc3 = pc.pack_images(rgb)
    src = torch.from_numpy(packed).to(cuda)
    old, old_u8 = ops.preprocess_images(src, torch.from_numpy(desc3), H, W, want_u8=True)                # ImageNet constants
    old_half, _ = ops.preprocess_images(src, torch.from_numpy(desc3), H, W, want_u8=True, mean=0.5, std=(0.5, 0.5, 0.5))
    desc4 = np.concatenate([desc3, np.full((3, 1), 3, np.int64)], 1)
    new, new_u8 = ops.preprocess_images(src, torch.from_numpy(desc4), H, W, want_u8=True)
    new_half, _ = run_px(ops, cuda, rgb, H, W)
    mixed_half, mixed_u8 = run_px(ops, cuda, [r[0] for r in refs], H, W)
    torch.cuda.synchronize()
    assert torch.equal(old, new) and torch.equal(old_u8, new_u8) and torch.equal(old_half, new_half)
    assert torch.equal(mixed_half, new_half) and torch.equal(mixed_u8, new_u8)
    for i, (_, want_u8, want_half) in enumerate(refs):
        assert torch.equal(old_u8[i].cpu(), want_u8)
        assert torch.equal(old[i].cpu(), pc.to_float(want_u8.numpy()))                    # today's call, today's bits
        assert torch.equal(old_half[i].cpu(), want_half)


def test_px_refusals_carry_a_message_and_launch_nothing(cuda):
    from canonicalsg2im_amd import _lib, ops
    _lib.prof_enable(1)
    _lib.prof_reset()
    try:
        src = torch.zeros(4 * 16 * 16 + 4, dtype=torch.uint8, device=cuda)
        with pytest.raises(RuntimeError, match="image 0 has 5 bytes per pixel, 3 or 4"):
            ops.preprocess_images(src, torch.tensor([[0, 16, 16, 5]]), 16, 16)
        with pytest.raises(RuntimeError, match="offset 8, 16 x 16 x 4 bytes. leaves the 1028 source bytes"):
            ops.preprocess_images(src, torch.tensor([[8, 16, 16, 4]]), 16, 16)
        with pytest.raises(RuntimeError, match="src must be 4-byte aligned"):
            ops.preprocess_images(src[1:], torch.tensor([[0, 16, 16, 4]]), 16, 16)
        with pytest.raises(RuntimeError, match="desc must be int64"):
            ops.preprocess_images(src, torch.tensor([[0, 16, 16, 4, 0]]), 16, 16)
        with pytest.raises(RuntimeError, match="mean must be a number or three"):
            ops.preprocess_images(src, torch.tensor([[0, 16, 16, 4]]), 16, 16, mean=(0.5, 0.5))
        torch.cuda.synchronize()
        assert "preprocess" not in _lib.prof_read()
        ops.preprocess_images(src, torch.tensor([[4, 16, 16, 4]]), 16, 16)
        assert _lib.prof_read()["preprocess"][1] == 1
    finally:
        _lib.prof_enable(0)
        _lib.prof_reset()


def test_captured_pair_replays_over_a_second_mixed_batch(cuda):
    """Both launches in a torch.cuda.graph; the replay reads pixels AND descriptor written into the captured buffers
    afterwards: other sizes, other bytes per pixel and other alignments per slot, bit-equal to eager and to the host."""
    from canonicalsg2im_amd import ops
    H = W = 64
    first = cc.batch_images("mixed", seed=3)
    second = [cc.batch_images("mixed", seed=4)[i] for i in (2, 0, 1)]
    p1, d1 = cc.pack_px(first)
    p2, d2 = cc.pack_px(second)
    assert p1.shape == p2.shape and d2[:, 1].max() <= d1[:, 1].max() and d2[:, 1].sum() <= d1[:, 1].sum()
    assert d1[2, 0] % 4 == 3 and d1[2, 3] == 4 and d2[2, 0] % 4 == 0 and d2[2, 3] == 3
    src = torch.from_numpy(p1).to(cuda)
    desc = torch.from_numpy(d1).to(cuda)
    out = torch.empty((3, 3, H, W), device=cuda)
    out_u8 = torch.empty((3, H, W, 3), device=cuda, dtype=torch.uint8)
    ws = torch.empty(3 * W * int(d1[:, 1].sum()), device=cuda, dtype=torch.uint8)
    kw = dict(want_u8=True, desc_host=torch.from_numpy(d1), out=out, out_u8=out_u8, workspace=ws, mean=0.5, std=0.5)
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        ops.preprocess_images(src, desc, H, W, **kw)                     # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(stream)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=stream):
        ops.preprocess_images(src, desc, H, W, **kw)
    graph.replay()
    torch.cuda.synchronize()
    eager1, eager1_u8 = run_px(ops, cuda, first, H, W)
    assert torch.equal(out, eager1) and torch.equal(out_u8, eager1_u8)
    src.copy_(torch.from_numpy(p2))
    desc.copy_(torch.from_numpy(d2))
    graph.replay()
    torch.cuda.synchronize()
    eager2, eager2_u8 = run_px(ops, cuda, second, H, W)
    assert torch.equal(out, eager2) and torch.equal(out_u8, eager2_u8)
    assert not torch.equal(eager1, eager2)
    for i, im in enumerate(second):
        assert torch.equal(out[i].cpu(), cc.to_float(pc.pil_resize_u8(cc.rgb_of(im), H, W)))


def test_captured_boxes_replay_over_a_second_batch(cuda):
    from canonicalsg2im_amd import ops
    g, objs, dev = _golden_on(cuda)
    bufs = [t[:11].clone() for t in dev]
    out = torch.empty((11, 10, 4), device=cuda)
    kw = dict(objs_host=objs[:11], counts_host=g["counts"][:11], out=out)
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        ops.clevr_boxes(*bufs, **kw)
    torch.cuda.current_stream().wait_stream(stream)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=stream):
        ops.clevr_boxes(*bufs, **kw)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out.cpu(), g["boxes"][:11])
    for b, t in zip(bufs, dev):
        b.copy_(t[11:])
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out.cpu(), g["boxes"][11:])


# ------------------------------------------------------------------------------------------------- 3. the dataset
def test_dataset_on_a_tiny_folder(cuda, tmp_path):
    pytest.importorskip("PIL")
    from canonicalsg2im_amd import train as T
    from canonicalsg2im_amd.scripts.train import build_parser, folder_builder, folder_dataset
    from canonicalsg2im_amd.sg2im.data import canonical_triplets
    from canonicalsg2im_amd.sg2im.data.packed_clevr import ClevrBatchBuilder
    from canonicalsg2im_amd.sg2im.data.packed_coco import CocoBatchBuilder
    base, scenes, pixels = cc.write_folder(str(tmp_path))
    args = build_parser().parse_args(["--dataset", "packed_clevr", "--dataroot", str(tmp_path), "--image_size", "64,64"])
    ds = folder_dataset(args, "train")
    assert len(ds) == 5 and [len(s["objects"]) for s in scenes] == [3, 4, 5, 6, 3]
    v = ds.vocab
    opt = T.make_opt(v, ["--image_size", "64,64", "--ngf", "8", "--ndf", "8", "--batch_size", "4", "--no_vgg_loss",
                         "--use_img_disc", "1", "--gconv_hidden_dim", "64", "--gconv_dim", "32", "--dataset", "packed_clevr",
                         "--loader_num_workers", "2"])
    torch.manual_seed(4)
    trainer = T.Trainer(opt, cuda)
    builder = folder_builder(ds, opt, trainer, cuda)
    assert isinstance(builder, ClevrBatchBuilder) and not isinstance(builder, CocoBatchBuilder) and builder.num_workers == 2
    # ---- one built batch against the host pipeline
    order = [3, 0, 2, 1]
    pending = builder.start(order)
    assert pending.desc[:, 3].tolist() == [4, 4, 4, 3] and bool((pending.desc[:, 0] % 4 == 0).all())
    batch = builder.finish(pending)
    torch.cuda.synchronize()
    imgs, bobjs, bboxes, triplets, conv_counts, ttype, masks, ids = batch
    assert masks is None and ids.tolist() == [13, 10, 12, 11]
    assert imgs.dtype == torch.float32 and tuple(imgs.shape) == (4, 3, 64, 64) and imgs.is_contiguous()
    for b, i in enumerate(order):
        px = pixels[scenes[i]["image_filename"]]
        assert px.shape[2] == len(cc.FOLDER_MODES[i])
        host = cc.to_float(pc.pil_resize_u8(cc.rgb_of(px), 64, 64))
        assert torch.equal(imgs[b].cpu(), host), "image %d of the batch is not the host pipeline's" % b
    O = 6
    assert tuple(bobjs.shape) == (4, O + 1, 4) and bobjs.dtype == torch.int64 and tuple(bboxes.shape) == (4, O + 1, 4)
    geom = np.zeros((4, O, 5))
    shape = np.zeros((4, O), np.int64)
    rot = np.zeros((4, 2))
    counts = np.asarray([len(scenes[i]["objects"]) for i in order])
    for b, i in enumerate(order):
        _, objs_i, geom_i, rot_i, _ = ds.load(i)
        n = counts[b]
        assert bobjs[b, :n].cpu().tolist() == objs_i.tolist() and bool((bobjs[b, n:] == 0).all())     # padding, __image__
        assert objs_i.tolist() == [[v["attributes"][a][o[a]] for a in ("shape", "color", "material", "size")]
                                   for o in scenes[i]["objects"]]
        geom[b, :n], shape[b, :n], rot[b] = geom_i.numpy(), objs_i[:, 0].numpy(), rot_i.numpy()
    want = torch.from_numpy(cc.boxes_fp64(geom, shape, rot, counts))
    assert torch.equal(bboxes[:, :O].cpu(), want) and bool((bboxes[:, O] == -1).all())
    assert bool((want[0] != -1).all()) and bool((want[1, 3:] == -1).all())
    centers = bboxes[..., :2] + 0.5 * bboxes[..., 2:]
    t2, c2, tt2 = canonical_triplets(bobjs, bboxes, centers, torch.as_tensor(counts + 1).to(cuda), v)
    assert torch.equal(triplets, t2) and torch.equal(conv_counts, c2) and torch.equal(ttype, tt2)
    assert triplets.shape[1] > O                           # the __in_image__ rows and location relations
    again = builder.build(order)                           # start + finish is build, tensor for tensor
    torch.cuda.synchronize()
    assert len(again) == len(batch) and all((a is None and b is None) or torch.equal(a, b) for a, b in zip(again, batch))
    # ---- five steps through the look-ahead iterator: graphs are captured and replayed while the workers decode
    assert trainer.graphs is not None and trainer.graphs.captures == 0
    for step, got in enumerate(builder.batches([order, order[::-1], order, order[::-1], order])):
        if step == 0:
            torch.cuda.synchronize()
            assert torch.equal(got[0], imgs) and torch.equal(got[2], bboxes) and torch.equal(got[3], triplets)
        if step == 1:
            assert got[7].tolist() == [11, 12, 10, 13]
        G, D = trainer.step(got)
        for k, val in list(G.items()) + list(D.items()):
            assert bool(torch.isfinite(val).all()), "step %d: %s" % (step, k)
    assert builder.steps == 5 and 0 <= builder.waited <= 5
    assert trainer.graphs.captures > 0 and trainer.graphs.replays > 0, (trainer.graphs.captures, trainer.graphs.replays)
    builder.close()
    # ---- a val split of another vocabulary is refused on the host; the same one passes; masks are refused with a reason
    from canonicalsg2im_amd.scripts import evaluate as val_cli
    cc.write_folder(str(tmp_path), split="val")
    assert len(val_cli.folder_val_set(args, v)) == 5
    other = dict(v, attributes=dict(v["attributes"], size={"__image__": 0, "small": 1}))
    with pytest.raises(SystemExit, match="attribute tables"):
        val_cli.folder_val_set(args, other)
    with pytest.raises(NotImplementedError, match="mask_size must be 0.*masks = None"):
        folder_dataset(build_parser().parse_args(["--dataset", "packed_clevr", "--dataroot", str(tmp_path), "--mask_size",
                                                  "16"]), "train")
