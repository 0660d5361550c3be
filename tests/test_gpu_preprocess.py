"""The input stage on a real MI355X: csrc/preprocess.hip against the host restatements of tests/preprocess_cases.py (which
tests/test_preprocess_cases.py pins to Pillow and torch on the CPU), and the COCO folder dataset that feeds it.

No tolerance anywhere: the resize is integer arithmetic on fp64-derived integer coefficients, and the float stage is three
correctly rounded fp32 operations; both sides are defined operation by operation, so the bytes and the bits are equal."""
import json
import os

import numpy as np
import pytest
import torch

import preprocess_cases as pc

gpu = pytest.mark.gpu            # per test: the epoch order at the end of the file is host-only

SUPPORTED = [c for c in pc.CASES if pc.supported(*c[:4])]


@pytest.fixture(scope="module")
def cuda():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device("cuda:0")


_REFERENCE = {}


def reference(case, H, W, seed=0):
    """(source image, resized uint8 (H,W,3), fp32 (3,H,W)) of a table row: computed once, shared, never written to."""
    key = (case[:2], H, W, seed)
    if key not in _REFERENCE:
        img = pc.case_image(case, seed)
        u8 = pc.pil_resize_u8(img, H, W)
        _REFERENCE[key] = (img, torch.from_numpy(u8), pc.to_float(u8))
    return _REFERENCE[key]


def run(ops, cuda, images, H, W, **kw):
    packed, desc = pc.pack_images(images)
    return ops.preprocess_images(torch.from_numpy(packed).to(cuda), torch.from_numpy(desc), H, W, want_u8=True, **kw)


def differing(a, b):
    return int((a != b).sum())


# --------------------------------------------------------------------------------------------- 1. the kernel
@gpu
def test_mixed_batch_equals_pillow_bytes_and_torch_bits(cuda):
    """Every supported row in ONE call of B = 7 (different sizes, passes skipped for some images and not for others; the
    rows meant for 64, 128 and 256 outputs all go to 64 x 64, a size every row supports), then at B = 1 at its own size."""
    from canonicalsg2im_amd import ops
    assert len(SUPPORTED) == 7
    refs = [reference(c, 64, 64) for c in SUPPORTED]
    f32, u8 = run(ops, cuda, [r[0] for r in refs], 64, 64)
    torch.cuda.synchronize()
    assert f32.dtype == torch.float32 and tuple(f32.shape) == (7, 3, 64, 64) and f32.is_contiguous()
    assert u8.dtype == torch.uint8 and tuple(u8.shape) == (7, 64, 64, 3) and u8.is_contiguous()
    for i, (c, r) in enumerate(zip(SUPPORTED, refs)):
        nb, nf = differing(u8[i].cpu(), r[1]), differing(f32[i].cpu(), r[2])
        print("mixed batch image %d %s -> 64x64: %d differing bytes, %d differing floats" % (i, pc.case_id(c), nb, nf))
        assert nb == 0 and nf == 0
        assert torch.equal(f32[i].cpu(), r[2])


@gpu
@pytest.mark.parametrize("case", SUPPORTED + pc.LIMIT_CASES, ids=pc.case_id)
def test_single_image_equals_pillow_bytes_and_torch_bits(cuda, case):
    from canonicalsg2im_amd import ops
    H, W = case[2:4]
    img, want_u8, want_f32 = reference(case, H, W)
    f32, u8 = run(ops, cuda, [img], H, W)
    only = ops.preprocess_images(torch.from_numpy(img.reshape(-1)).to(cuda),
                                 torch.tensor([[0, img.shape[0], img.shape[1]]]), H, W)
    torch.cuda.synchronize()
    nb, nf = differing(u8[0].cpu(), want_u8), differing(f32[0].cpu(), want_f32)
    print("%s: %d differing bytes of %d, %d differing floats" % (pc.case_id(case), nb, want_u8.numel(), nf))
    assert nb == 0
    assert torch.equal(f32[0].cpu(), want_f32)
    assert torch.equal(only, f32), "the call without the uint8 output gives other floats"


@gpu
@pytest.mark.parametrize("hw,HW", [((23, 31), (10, 13)), ((9, 70), (9, 67)), ((40, 7), (5, 7))],
                         ids=["both_axes", "height_kept", "width_kept"])
def test_widths_that_are_no_multiple_of_four_take_the_narrow_stores(cuda, hw, HW):
    """W % 4 != 0: rows of the planes and of the workspace are not dword-aligned, and the last quad of a row is partial.
    The two images of the batch make the second one's workspace start at an odd byte."""
    from canonicalsg2im_amd import ops
    cases = [(hw[0], hw[1]) + HW, (hw[0] + 2, hw[1] + (0 if hw[1] == HW[1] else 3)) + HW]
    refs = [reference(c, HW[0], HW[1], seed=2) for c in cases]
    f32, u8 = run(ops, cuda, [r[0] for r in refs], HW[0], HW[1])
    torch.cuda.synchronize()
    for i, r in enumerate(refs):
        assert differing(u8[i].cpu(), r[1]) == 0
        assert torch.equal(f32[i].cpu(), r[2])


@gpu
def test_byte_ramp_isolates_the_float_stage(cuda):
    """16 x 16 -> 16 x 16 (both passes skipped): every byte value in every channel, bit-equal to torch on the host, with
    and without the normalisation; without it the result is exactly byte / 255."""
    from canonicalsg2im_amd import ops
    ramp = np.repeat(np.arange(256, dtype=np.uint8).reshape(16, 16, 1), 3, axis=2)
    f32, u8 = run(ops, cuda, [ramp], 16, 16)
    plain, _ = run(ops, cuda, [ramp], 16, 16, normalize=False)
    torch.cuda.synchronize()
    assert torch.equal(u8[0].cpu(), torch.from_numpy(ramp))
    assert torch.equal(f32[0].cpu(), pc.to_float(ramp))
    assert torch.equal(plain[0].cpu(), pc.to_float(ramp, mean=None))
    exact = torch.from_numpy((np.moveaxis(ramp, -1, 0).astype(np.float64) / 255.0).astype(np.float32))
    assert torch.equal(plain[0].cpu(), exact)


@gpu
def test_normalize_false_on_a_resized_image(cuda):
    from canonicalsg2im_amd import ops
    case = SUPPORTED[2]
    img, want_u8, _ = reference(case, 64, 64)
    plain, u8 = run(ops, cuda, [img], 64, 64, normalize=False)
    torch.cuda.synchronize()
    assert torch.equal(u8[0].cpu(), want_u8)
    assert torch.equal(plain[0].cpu(), pc.to_float(want_u8.numpy(), mean=None))


@gpu
def test_refusals_carry_a_message_and_launch_nothing(cuda):
    from canonicalsg2im_amd import _lib, ops
    _lib.prof_enable(1)
    _lib.prof_reset()
    try:
        beyond = [c for c in pc.CASES if not pc.supported(*c[:4])]
        assert [c[:4] for c in beyond] == [(17, 1000, 8, 8)]
        img = pc.case_image(beyond[0])
        with pytest.raises(RuntimeError, match="shrinks an axis by more than 64"):
            run(ops, cuda, [img], 8, 8)
        src = torch.zeros(3 * 16 * 16, dtype=torch.uint8, device=cuda)
        with pytest.raises(RuntimeError, match="image 1 is 0 x 16"):
            ops.preprocess_images(src, torch.tensor([[0, 16, 16], [0, 0, 16]]), 16, 16)
        with pytest.raises(RuntimeError, match="leaves the 768 source bytes"):
            ops.preprocess_images(src, torch.tensor([[3, 16, 16]]), 16, 16)
        with pytest.raises(RuntimeError, match="no CPU path"):
            ops.preprocess_images(src.cpu(), torch.tensor([[0, 16, 16]]), 16, 16)
        shifted = torch.empty(3 * 16 * 16 + 1, device=cuda)[1:].view(1, 3, 16, 16)       # contiguous, 4 bytes off
        with pytest.raises(RuntimeError, match="out must be 16-byte aligned"):
            ops.preprocess_images(src, torch.tensor([[0, 16, 16]]), 16, 16, out=shifted)
        torch.cuda.synchronize()
        assert "preprocess" not in _lib.prof_read()
        ops.preprocess_images(src, torch.tensor([[0, 16, 16]]), 16, 16)
        assert _lib.prof_read()["preprocess"][1] == 1           # the table does see a call that launches
    finally:
        _lib.prof_enable(0)
        _lib.prof_reset()


# (h, w) of the captured batch and of the batch replayed over it: as many bytes, no taller, no more workspace
REPLAYS = {
    "reordered": ([(37, 53), (300, 64), (64, 64)], [(300, 64), (64, 64), (37, 53)]),
    # captured where EVERY width is already W: the horizontal launch must be in the graph all the same
    "widths_appear": ([(300, 64), (64, 64), (40, 64)], [(64, 64), (300, 64), (32, 80)]),
}


@gpu
@pytest.mark.parametrize("name", sorted(REPLAYS))
def test_captured_launches_replay_over_a_second_batch(cuda, name):
    """Both launches in a torch.cuda.graph on one stream; the replay reads pixels AND descriptor written into the captured
    buffers afterwards, bit-equal to eager."""
    from canonicalsg2im_amd import ops
    H = W = 64
    first = [pc.case_image(c, seed=3) for c in REPLAYS[name][0]]
    second = [pc.case_image(c, seed=4) for c in REPLAYS[name][1]]
    p1, d1 = pc.pack_images(first)
    p2, d2 = pc.pack_images(second)
    assert p1.shape == p2.shape and d2[:, 1].max() <= d1[:, 1].max() and d2[:, 1].sum() <= d1[:, 1].sum()
    src = torch.from_numpy(p1).to(cuda)
    desc = torch.from_numpy(d1).to(cuda)
    out = torch.empty((3, 3, H, W), device=cuda)
    out_u8 = torch.empty((3, H, W, 3), device=cuda, dtype=torch.uint8)
    ws = torch.empty(3 * W * int(d1[:, 1].sum()), device=cuda, dtype=torch.uint8)
    kw = dict(want_u8=True, desc_host=torch.from_numpy(d1), out=out, out_u8=out_u8, workspace=ws)
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
    eager1, eager1_u8 = run(ops, cuda, first, H, W)
    assert torch.equal(out, eager1) and torch.equal(out_u8, eager1_u8)
    src.copy_(torch.from_numpy(p2))
    desc.copy_(torch.from_numpy(d2))
    graph.replay()
    torch.cuda.synchronize()
    eager2, eager2_u8 = run(ops, cuda, second, H, W)
    assert torch.equal(out, eager2) and torch.equal(out_u8, eager2_u8)
    assert not torch.equal(eager1, eager2)
    for i, im in enumerate(second):
        assert torch.equal(out[i].cpu(), pc.to_float(pc.pil_resize_u8(im, H, W)))


# --------------------------------------------------------------------------------------------- 2. the dataset
CATEGORIES_THINGS = [{"id": 1, "name": "person"}, {"id": 3, "name": "car"}, {"id": 17, "name": "cat"}]
CATEGORIES_STUFF = [{"id": 92, "name": "sky"}, {"id": 95, "name": "grass"}, {"id": 183, "name": "other"}]
SIZES = [(48, 64), (37, 53), (64, 64), (80, 40), (33, 47), (64, 30)]      # (h, w) of images 1 .. 6


def _box(W, H, x, y, w, h):
    return [x * W, y * H, w * W, h * H]


def write_folder(root):
    """6 seeded PNGs and the two annotation files.  By construction:
    image 1 .. 3  three kept objects each (things and stuff mixed), sizes that resize, upscale and pass through;
    image 4       no stuff annotation at all                           -> dropped (stuff_only);
    image 5       kept objects + one box of 1% of the image            -> the small box is dropped, the image stays;
                  + one stuff annotation of category "other"           -> that object is dropped;
    image 6       one kept object only                                 -> below min_objects = 2, dropped."""
    from PIL import Image
    os.makedirs(os.path.join(root, "images"))
    images, pixels = [], {}
    for i, (h, w) in enumerate(SIZES, start=1):
        name = "img_%02d.png" % i
        px = np.random.default_rng(50 + i).integers(0, 256, size=(h, w, 3), dtype=np.uint8)
        Image.fromarray(px, "RGB").save(os.path.join(root, "images", name))
        images.append({"id": 100 + i, "file_name": name, "width": w, "height": h})
        pixels[100 + i] = px
    size = {100 + i: (w, h) for i, (h, w) in enumerate(SIZES, start=1)}
    things, stuff = [], []

    def add(dst, image, cat, x, y, w, h):
        dst.append({"id": len(things) + len(stuff) + 1, "image_id": image, "category_id": cat,
                    "bbox": _box(size[image][0], size[image][1], x, y, w, h)})

    for image in (101, 102, 103):
        add(things, image, 1, 0.10, 0.20, 0.30, 0.50)
        add(things, image, 17, 0.55, 0.40, 0.35, 0.45)
        add(stuff, image, 92, 0.00, 0.00, 1.00, 0.35)
    add(things, 104, 3, 0.1, 0.1, 0.5, 0.5)
    add(things, 104, 1, 0.5, 0.5, 0.4, 0.4)
    add(things, 105, 3, 0.05, 0.55, 0.40, 0.40)
    add(things, 105, 1, 0.60, 0.10, 0.10, 0.10)          # 1% of the image: below min_object_size = 0.02
    add(stuff, 105, 95, 0.00, 0.50, 1.00, 0.50)
    add(stuff, 105, 183, 0.20, 0.20, 0.50, 0.50)         # "other"
    add(things, 106, 1, 0.2, 0.2, 0.5, 0.5)
    add(stuff, 106, 183, 0.0, 0.0, 0.9, 0.9)             # "other": image 106 keeps one object
    inst = os.path.join(root, "instances.json")
    stf = os.path.join(root, "stuff.json")
    with open(inst, "w") as f:
        json.dump({"images": images, "categories": CATEGORIES_THINGS, "annotations": things}, f)
    with open(stf, "w") as f:
        json.dump({"images": images, "categories": CATEGORIES_STUFF, "annotations": stuff}, f)
    return os.path.join(root, "images"), inst, stf, pixels, things, stuff


@gpu
def test_dataset_on_a_tiny_folder(cuda, tmp_path):
    pytest.importorskip("PIL")
    from canonicalsg2im_amd import train as T
    from canonicalsg2im_amd.sg2im.data import canonical_triplets
    from canonicalsg2im_amd.sg2im.data.packed_coco import CocoBatchBuilder, PackedCocoSceneGraphDataset
    image_dir, inst, stf, pixels, things, stuff = write_folder(str(tmp_path))
    ds = PackedCocoSceneGraphDataset(image_dir, inst, stf, image_size=(64, 64), min_object_size=0.02, min_objects=2,
                                     max_objects=8)
    # ---- filters
    assert ds.image_ids == [101, 102, 103, 105] and len(ds) == 4
    assert [o["category_id"] for o in ds.image_id_to_objects[105]] == [3, 95]
    assert [o["category_id"] for o in ds.image_id_to_objects[101]] == [1, 17, 92]
    assert 104 not in ds.image_id_to_objects and 104 not in ds.image_id_to_filename
    assert len(PackedCocoSceneGraphDataset(image_dir, inst, stf, image_size=(64, 64), min_objects=2, max_objects=8,
                                           max_samples=3)) == 3
    with_other = PackedCocoSceneGraphDataset(image_dir, inst, stf, image_size=(64, 64), min_objects=2, max_objects=8,
                                             include_other=True)
    assert with_other.image_ids == [101, 102, 103, 105, 106]
    only_people = PackedCocoSceneGraphDataset(image_dir, inst, stf, image_size=(64, 64), min_objects=1, max_objects=8,
                                              instance_whitelist=["person"], stuff_whitelist=["sky"])
    assert [o["category_id"] for o in only_people.image_id_to_objects[101]] == [1, 92]
    # ---- vocabulary
    v = ds.vocab
    assert v["object_name_to_idx"] == {"person": 1, "car": 3, "cat": 17, "sky": 92, "grass": 95, "other": 183, "__image__": 0}
    assert len(v["object_idx_to_name"]) == 184 and v["object_idx_to_name"][0] == "__image__"
    assert v["object_idx_to_name"][17] == "cat" and v["object_idx_to_name"][2] == "NONE"
    assert v["pred_idx_to_name"] == ["__padding__", "__in_image__", "__below__", "__above__", "__left of__", "__right of__",
                                     "__inside__", "__surrounding__"]
    assert v["attributes"] == {"objects": v["object_name_to_idx"]}
    assert v["reverse_attributes"]["objects"][92] == "sky"
    # ---- one sample on the host: the boxes are the annotation over the DECODED size
    px, objs, boxes, image_id = ds.load(3)
    assert image_id == 105 and np.array_equal(px, pixels[105]) and objs.tolist() == [3, 95]
    HH, WW = SIZES[4]
    want = torch.stack([torch.FloatTensor([x / WW, y / HH, w / WW, h / HH])
                        for x, y, w, h in (o["bbox"] for o in ds.image_id_to_objects[105])])
    assert torch.equal(boxes, want)
    # ---- one built batch
    opt = T.make_opt(v, ["--image_size", "64,64", "--ngf", "8", "--ndf", "8", "--batch_size", "4", "--no_vgg_loss",
                         "--use_img_disc", "1", "--gconv_hidden_dim", "64", "--gconv_dim", "32", "--dataset", "packed_coco"])
    torch.manual_seed(4)
    trainer = T.Trainer(opt, cuda)
    builder = CocoBatchBuilder(ds, opt, trainer, cuda, num_workers=2)
    order = [3, 0, 2, 1]
    pending = builder.start(order)
    assert pending.desc.shape == (4, 3)                   # the three-column entry, every picture as RGB, back to back
    assert pending.desc.tolist() == [[sum(3 * h * w for h, w in (pixels[ds.image_ids[j]].shape[:2] for j in order[:b]))] +
                                     list(pixels[ds.image_ids[i]].shape[:2]) for b, i in enumerate(order)]
    batch = builder.finish(pending)
    torch.cuda.synchronize()
    imgs, bobjs, bboxes, triplets, conv_counts, ttype, masks, ids = batch
    assert masks is None and ids.tolist() == [105, 101, 103, 102]
    assert imgs.dtype == torch.float32 and tuple(imgs.shape) == (4, 3, 64, 64) and imgs.is_contiguous()
    for b, i in enumerate(order):
        host = pc.to_float(pc.pil_resize_u8(pixels[ds.image_ids[i]], 64, 64))
        assert torch.equal(imgs[b].cpu(), host), "image %d of the batch is not the host pipeline's" % b
    assert tuple(bobjs.shape) == (4, 4, 1) and tuple(bboxes.shape) == (4, 4, 4)           # 3 objects + __image__
    assert bobjs[0, :, 0].tolist() == [3, 95, 0, 0] and bobjs[1, :, 0].tolist() == [1, 17, 92, 0]
    assert torch.equal(bboxes[0, :2].cpu(), want) and bool((bboxes[0, 2:] == -1).all())
    n = torch.tensor([3, 4, 4, 4])
    centers = bboxes[..., :2] + 0.5 * bboxes[..., 2:]
    t2, c2, tt2 = canonical_triplets(bobjs, bboxes, centers, n.to(cuda), v)
    assert torch.equal(triplets, t2) and torch.equal(conv_counts, c2) and torch.equal(ttype, tt2)
    # ---- the look-ahead iterator: the same batch first, then steps with HIP graphs captured while the workers decode.
    # Trainer.step captures a shape key at its second sighting (graphs.py): step 2 below opens its captures while the
    # worker threads hold batch 3.  They make no HIP call, so the captures go through, and the later steps replay.
    assert trainer.graphs is not None and trainer.graphs.captures == 0
    it = builder.batches([order, order[::-1], order, order[::-1], order])
    for step, got in enumerate(it):
        if step == 0:
            torch.cuda.synchronize()
            assert torch.equal(got[0], imgs) and torch.equal(got[3], triplets)
        if step == 1:
            assert got[7].tolist() == [102, 103, 101, 105]
        G, D = trainer.step(got)
        for k, val in list(G.items()) + list(D.items()):
            assert bool(torch.isfinite(val).all()), "step %d: %s" % (step, k)
    assert builder.steps == 5 and 0 <= builder.waited <= 5
    assert trainer.graphs.captures > 0 and trainer.graphs.replays > 0, (trainer.graphs.captures, trainer.graphs.replays)
    # ---- two more training steps on the batch built directly
    for _ in range(2):
        G, D = trainer.step(batch)
        for k, val in list(G.items()) + list(D.items()):
            assert bool(torch.isfinite(val).all()), k
    builder.close()
    # ---- masks are out of scope, and the message says why
    with pytest.raises(NotImplementedError, match="mask_size must be 0.*box centres"):
        PackedCocoSceneGraphDataset(image_dir, inst, stf, image_size=(64, 64), mask_size=1)


def test_epoch_order_is_seeded_and_ranks_take_disjoint_slices():
    from canonicalsg2im_amd.sg2im.data.loader import epoch_batches
    n, per_rank, world = 37, 3, 2
    a = [epoch_batches(n, per_rank, r, world, seed=5, epoch=2) for r in range(world)]
    b = [epoch_batches(n, per_rank, r, world, seed=5, epoch=2) for r in range(world)]
    assert a == b
    assert a != [epoch_batches(n, per_rank, r, world, seed=5, epoch=3) for r in range(world)]
    assert a != [epoch_batches(n, per_rank, r, world, seed=6, epoch=2) for r in range(world)]
    assert len(a[0]) == len(a[1]) == n // (per_rank * world)              # the ragged tail is dropped: equal steps per rank
    flat = [[i for batch in r for i in batch] for r in a]
    assert all(len(batch) == per_rank for r in a for batch in r)
    assert not set(flat[0]) & set(flat[1])
    assert len(set(flat[0]) | set(flat[1])) == len(flat[0]) + len(flat[1]) == 36
    assert set(flat[0]) | set(flat[1]) <= set(range(n))
    whole = epoch_batches(12, 4, 0, 1, seed=1, epoch=0)
    assert sorted(i for batch in whole for i in batch) == list(range(12))
    assert [i for batch in epoch_batches(12, 4, 0, 1, seed=1, epoch=0, shuffle=False) for i in batch] == list(range(12))
