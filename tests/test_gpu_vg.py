"""The Visual Genome input stage on a real MI355X: csrc/vg.hip against the reference's recorded samples
(tests/golden/vg_samples.npz) and the numpy restatement of tests/vg_cases.py (which tests/test_vg_cases.py pins to the
reference on the CPU), and the folder dataset that feeds it, csg_preprocess_px and csg_canon_general_* together.

No tolerance anywhere: a box is four fp64 divisions rounded once to fp32, the resize is integer arithmetic, the float stage
is three correctly rounded fp32 operations, the graph is integers; both sides are defined operation by operation, so the
bits are equal."""
import ctypes
import os
import random

import numpy as np
import pytest
import torch

import preprocess_cases as pc
import vg_cases as vc

pytestmark = pytest.mark.gpu

NUM_NAMES = 179
MODEL = ["--image_size", "64,64", "--ngf", "8", "--ndf", "8", "--batch_size", "4", "--no_vgg_loss", "--use_img_disc", "1",
         "--gconv_hidden_dim", "64", "--gconv_dim", "32", "--dataset", "packed_vg", "--loader_num_workers", "2",
         "--min_objects", "1"]


@pytest.fixture(scope="module")
def cuda():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def folder(tmp_path_factory):
    """(dataroot, base, decoded pictures, the host pipeline's 64 x 64 fp32 images): written and computed once, shared, never
    written to."""
    root = str(tmp_path_factory.mktemp("vgroot"))
    base, decoded = vc.write_folder(root)
    vc.write_folder(root, split="val")
    return root, base, decoded, [vc.to_float(pc.pil_resize_u8(px, 64, 64)) for px in decoded]


def _dataset(base, si):
    from canonicalsg2im_amd.sg2im.data.packed_vg import PackedVGDataset
    s = vc.golden()[0]["settings"][si]
    return PackedVGDataset(os.path.join(base, "train.npz"), os.path.join(base, "images"), os.path.join(base, "vocab.json"),
                           image_size=(64, 64), max_objects=s["max_objects"], use_orphaned_objects=bool(s["use_orphaned_objects"]),
                           include_relationships=bool(s["include_relationships"]))


def _run(ops, cuda, rows, sizes, counts, **kw):
    rows, sizes, counts = (torch.from_numpy(np.array(a)) for a in (rows, sizes, counts))
    objs, boxes = ops.vg_rows(rows.to(cuda), sizes.to(cuda), counts.to(cuda), NUM_NAMES, rows_host=rows, sizes_host=sizes,
                              counts_host=counts, **kw)
    torch.cuda.synchronize()
    return objs.cpu().numpy(), boxes.cpu().numpy()


def _same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype == np.float32 and np.array_equal(a.view(np.uint32), b.view(np.uint32))


# ------------------------------------------------------------------------------------------------- 1. the launch
@pytest.mark.parametrize("si", range(6), ids=vc.setting_id)
def test_rows_equal_the_reference_bit_for_bit(cuda, folder, si):
    from canonicalsg2im_amd import ops
    meta, g = vc.golden()
    s = meta["settings"][si]
    picks = vc.select_all(_dataset(folder[1], si), si)
    rows, counts = vc.padded_rows(g, s["samples"], [chosen for chosen, _ in picks])
    sizes = g["sizes"][s["samples"]]
    objs, boxes = _run(ops, cuda, rows, sizes, counts)
    want_objs, want_boxes = g["s%d_objs" % si].astype(np.int64), g["s%d_boxes" % si]
    B, O = rows.shape[:2]
    assert (B, O + 1) == want_objs.shape and objs.shape == (B, O, 1) and objs.dtype == np.int64
    got_objs, got_boxes = vc.with_image_row(objs[..., 0], boxes)
    differing = int((got_boxes.view(np.uint32) != want_boxes.view(np.uint32)).any(-1).sum())
    print("%s (B,O) = (%d,%d): %d of %d box rows differ from the reference's bits" % (vc.setting_id(si), B, O, differing, B * (O + 1)))
    assert differing == 0 and np.array_equal(got_objs, want_objs)
    read_back = ops.vg_rows(*(torch.from_numpy(np.array(a)).to(cuda) for a in (rows, sizes, counts)), NUM_NAMES)
    assert np.array_equal(read_back[0].cpu().numpy(), objs) and _same_bits(read_back[1].cpu().numpy(), boxes)


def test_two_blocks_and_one_row_equal_the_restatement(cuda):
    """(B,O) = (3,101): 303 rows, a full block of 256 lanes and a ragged one, counts 0, 101 and 37; and (1,1)."""
    from canonicalsg2im_amd import ops
    rng = np.random.default_rng(11)
    rows = rng.integers(0, 5000, size=(3, 101, 5)).astype(np.int32)
    rows[..., 0] = rng.integers(1, NUM_NAMES, size=(3, 101))
    rows[1, 100] = (NUM_NAMES - 1, 0, 0, 1, 1)
    sizes = np.asarray([[333, 500], [3001, 4999], [1, 7]], np.int64)
    counts = np.asarray([0, 101, 37], np.int64)
    objs, boxes = _run(ops, cuda, rows, sizes, counts)
    want_objs, want_boxes = vc.rows_fp64(rows, sizes, counts, NUM_NAMES)
    assert np.array_equal(objs[..., 0], want_objs) and _same_bits(boxes, want_boxes)
    assert (objs[0] == 0).all() and (boxes[0] == -1).all() and (objs[1] > 0).all() and (boxes[2, 37:] == -1).all()
    assert objs[1, 100, 0] == NUM_NAMES - 1 and boxes[1, 100].tolist() == [0.0, 0.0, np.float32(1 / 4999), np.float32(1 / 3001)]
    one = np.asarray([[[5, 3, 4, 7, 9]]], np.int32)
    objs, boxes = _run(ops, cuda, one, np.asarray([[11, 13]], np.int64), np.asarray([1], np.int64))
    assert objs.tolist() == [[[5]]] and _same_bits(boxes, np.asarray([[[3 / 13, 4 / 11, 7 / 13, 9 / 11]]]).astype(np.float32))


def test_refusals_carry_a_message_and_launch_nothing(cuda):
    from canonicalsg2im_amd import _lib, ops
    B, O = 2, 3
    rows = torch.tensor([[[4, 1, 2, 3, 4]] * O] * B, dtype=torch.int32)
    sizes = torch.tensor([[20, 30]] * B, dtype=torch.int64)
    counts = torch.tensor([3, 2], dtype=torch.int64)
    dev = [t.to(cuda) for t in (rows, sizes, counts)]
    out_objs = torch.full((B, O, 1), 77, dtype=torch.int64, device=cuda)
    out_boxes = torch.full((B, O, 4), 9.0, device=cuda)

    def call(r=rows, s=sizes, c=counts, names=NUM_NAMES, **kw):
        kw.setdefault("out_objs", out_objs)
        kw.setdefault("out_boxes", out_boxes)
        return ops.vg_rows(r.to(cuda), s.to(cuda), c.to(cuda), names, rows_host=r, sizes_host=s, counts_host=c, **kw)

    _lib.prof_enable(1)
    _lib.prof_reset()
    try:
        for shape in ((1025, 1), (0, 1), (1, 256), (1, 0)):
            b, o = shape
            with pytest.raises(RuntimeError, match="bad shape B=%d O=%d " % shape):
                call(torch.ones((b, o, 5), dtype=torch.int32), torch.ones((b, 2), dtype=torch.int64),
                     torch.zeros(b, dtype=torch.int64), out_objs=None, out_boxes=None)
        for bad in (4, -1):
            c = counts.clone()
            c[1] = bad
            with pytest.raises(RuntimeError, match="sample 1 has %d objects, 0 .. O = 3" % bad):
                call(c=c)
        for bad, text in (((0, 30), "0 x 30"), ((20, -2), "20 x -2")):
            s = sizes.clone()
            s[0] = torch.tensor(bad)
            with pytest.raises(RuntimeError, match="the picture of sample 0 is %s .HH x WW., at least 1 x 1" % text):
                call(s=s)
        for bad in (0, NUM_NAMES, -1):
            r = rows.clone()
            r[1, 1, 0] = bad
            with pytest.raises(RuntimeError, match="object 1 of sample 1 has name id %d, 1 .. 178" % bad):
                call(r=r)
        r = rows.clone()
        r[1, 2, 0] = 9999                                  # sample 1 has two objects: row 2 is padding, its name is not looked at
        with pytest.raises(RuntimeError, match="1 object names, 2 .. "):
            call(names=1)
        misaligned = torch.full((B * O * 4 + 1,), 9.0, device=cuda)[1:].view(B, O, 4)
        with pytest.raises(RuntimeError, match="boxes must be 16-byte aligned"):
            call(out_boxes=misaligned)
        host = [ctypes.c_void_p(t.data_ptr()) for t in (rows, sizes, counts)]
        args = [_lib.ptr(t) for t in dev] + host + [NUM_NAMES, B, O, _lib.ptr(out_objs), _lib.ptr(out_boxes), _lib.stream()]
        for k in (0, 1, 2, 3, 4, 5, 9, 10):
            with pytest.raises(RuntimeError, match="null operand"):
                _lib.check(_lib.lib.csg_vg_rows(*[None if j == k else a for j, a in enumerate(args)]), "vg_rows")
        with pytest.raises(RuntimeError, match="no CPU path"):
            ops.vg_rows(rows, dev[1], dev[2], NUM_NAMES)
        with pytest.raises(RuntimeError, match="rows must be contiguous torch.int32"):
            ops.vg_rows(dev[0].long(), dev[1], dev[2], NUM_NAMES)
        torch.cuda.synchronize()
        assert "vg_rows" not in _lib.prof_read()
        assert bool((out_objs == 77).all()) and bool((out_boxes == 9.0).all()) and bool((misaligned == 9.0).all())
        got = call(r=r)                                    # the padding-row name: accepted, and written as padding
        torch.cuda.synchronize()
        assert _lib.prof_read()["vg_rows"][1] == 1
        want = vc.rows_fp64(r.numpy(), sizes.numpy(), counts.numpy(), NUM_NAMES)
        assert np.array_equal(got[0].cpu().numpy()[..., 0], want[0]) and _same_bits(got[1].cpu().numpy(), want[1])
        assert got[0].data_ptr() == out_objs.data_ptr() and got[0][1, 2, 0] == 0
    finally:
        _lib.prof_enable(0)
        _lib.prof_reset()


def test_a_stale_device_row_becomes_a_padding_row(cuda, folder):
    """The host copies pass, the device buffers disagree (as under a replayed graph whose buffer was not refreshed): the row
    with the impossible name and the rows of the picture with an impossible size are padding; nothing else changes."""
    from canonicalsg2im_amd import ops
    _, g = vc.golden()
    picks = vc.select_all(_dataset(folder[1], 0), 0)
    rows, counts = vc.padded_rows(g, range(4), [chosen for chosen, _ in picks])
    rows_t, sizes_t, counts_t = (torch.from_numpy(np.array(a)) for a in (rows, g["sizes"], counts))
    stale_rows, stale_sizes = rows_t.to(cuda), sizes_t.to(cuda)
    stale_rows[1, 4, 0] = NUM_NAMES
    stale_rows[2, 0, 0] = -7
    stale_sizes[3, 1] = 0
    objs, boxes = ops.vg_rows(stale_rows, stale_sizes, counts_t.to(cuda), NUM_NAMES, rows_host=rows_t, sizes_host=sizes_t,
                              counts_host=counts_t)
    want_objs, want_boxes = vc.rows_fp64(rows, g["sizes"], counts, NUM_NAMES)
    want_objs, want_boxes = want_objs.copy(), want_boxes.copy()
    for where in ((1, 4), (2, 0), (3, slice(None))):
        want_objs[where] = 0
        want_boxes[where] = -1
    assert np.array_equal(objs.cpu().numpy()[..., 0], want_objs) and _same_bits(boxes.cpu().numpy(), want_boxes)
    assert (want_objs[0] > 0).sum() == 5 and (want_objs[1] > 0).sum() == 11 and (want_objs[2] > 0).sum() == 23


def test_captured_launch_replays_over_a_second_batch(cuda, folder):
    from canonicalsg2im_amd import ops
    _, g = vc.golden()
    picks = vc.select_all(_dataset(folder[1], 0), 0)
    rows, counts = vc.padded_rows(g, range(4), [chosen for chosen, _ in picks])
    first = [torch.from_numpy(np.array(a)) for a in (rows, g["sizes"], counts)]
    second = [first[0].flip(0).contiguous(), first[1].flip(0).contiguous(), first[2].flip(0).contiguous()]
    second[0][..., 1:] += 3
    bufs = [t.to(cuda) for t in first]
    out_objs = torch.empty((4, rows.shape[1], 1), dtype=torch.int64, device=cuda)
    out_boxes = torch.empty((4, rows.shape[1], 4), device=cuda)
    kw = dict(rows_host=first[0], sizes_host=first[1], counts_host=first[2], out_objs=out_objs, out_boxes=out_boxes)
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        ops.vg_rows(*bufs, NUM_NAMES, **kw)                              # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(stream)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=stream):
        ops.vg_rows(*bufs, NUM_NAMES, **kw)
    graph.replay()
    torch.cuda.synchronize()
    want = vc.rows_fp64(rows, g["sizes"], counts, NUM_NAMES)
    assert np.array_equal(out_objs.cpu().numpy()[..., 0], want[0]) and _same_bits(out_boxes.cpu().numpy(), want[1])
    for b, t in zip(bufs, second):
        b.copy_(t)
    graph.replay()
    torch.cuda.synchronize()
    want2 = vc.rows_fp64(*(t.numpy() for t in second), NUM_NAMES)
    assert np.array_equal(out_objs.cpu().numpy()[..., 0], want2[0]) and _same_bits(out_boxes.cpu().numpy(), want2[1])
    assert not np.array_equal(want[1], want2[1])


# ------------------------------------------------------------------------------------------------- 2. the dataset
def _args(vocab, extra=()):
    from canonicalsg2im_amd import train as T
    return T.make_opt(vocab, MODEL + list(extra))


@pytest.mark.parametrize("si", [0, 1, 4, 5], ids=vc.setting_id)
def test_whole_batch_equals_the_reference_collate(cuda, folder, si):
    """VGBatchBuilder.build over the tiny folder, drawing from the seeded `random` module as the reference did: objects and
    boxes with the __image__ row, triplets and triplet types are the reference's collate output; the images are the host
    pipeline's, the L, RGBA and JPEG pictures included."""
    from canonicalsg2im_amd.scripts.train import folder_builder
    from canonicalsg2im_amd.sg2im.data.packed_vg import VGBatchBuilder
    meta, g = vc.golden()
    s = meta["settings"][si]
    ds = _dataset(folder[1], si)
    opt = _args(ds.vocab, ["--learned_transitivity", str(s["learned_transitivity"])])
    builder = folder_builder(ds, opt, None, cuda, rng=random)
    assert isinstance(builder, VGBatchBuilder) and builder.num_workers == 2
    random.seed(s["seed"])
    pending = builder.start(s["samples"])
    assert pending.desc[:, 3].tolist() == [3, 3, 4, 3] and bool((pending.desc[:, 0] % 4 == 0).all())
    assert pending.sizes.tolist() == g["sizes"].tolist() and pending.rel.shape[2] == 3 and not pending.rel.is_cuda
    imgs, objs, boxes, triplets, conv_counts, ttype, masks, ids = builder.finish(pending)
    torch.cuda.synchronize()
    builder.close()
    assert masks is None and ids.tolist() == meta["image_ids"]
    assert objs.dtype == torch.int64 and np.array_equal(objs.cpu().numpy()[..., 0], g["s%d_objs" % si].astype(np.int64))
    assert _same_bits(boxes.cpu().numpy(), g["s%d_boxes" % si])
    assert triplets.dtype == torch.int64 and tuple(triplets.shape) == tuple(s["triplets"])
    assert np.array_equal(triplets.cpu().numpy(), g["s%d_triplets" % si].astype(np.int64))
    assert np.array_equal(ttype.cpu().numpy(), g["s%d_tt" % si].astype(np.int64)) and not bool(conv_counts.any())
    assert imgs.dtype == torch.float32 and tuple(imgs.shape) == (4, 3, 64, 64) and imgs.is_contiguous()
    for b in range(4):
        nf = int((imgs[b].cpu() != folder[3][b]).sum())
        print("picture %d (%s, %s): %d differing floats" % (b, vc.FOLDER_FILES[b], vc.FOLDER_MODES[b], nf))
        assert nf == 0 and torch.equal(imgs[b].cpu(), folder[3][b])


def test_steps_on_built_batches_and_the_look_ahead(cuda, folder):
    from canonicalsg2im_amd import train as T
    from canonicalsg2im_amd.scripts.train import build_parser, folder_builder, folder_dataset
    ds = folder_dataset(build_parser().parse_args(["--dataset", "packed_vg", "--dataroot", folder[0], "--image_size", "64,64",
                                                   "--min_objects", "1"]), "train")
    assert len(ds) == 4 and ds.max_objects == 100
    opt = _args(ds.vocab)
    torch.manual_seed(4)
    trainer = T.Trainer(opt, cuda)
    lists = [[3, 0, 2, 1], [1, 2, 0, 3]]
    builder = folder_builder(ds, opt, trainer, cuda, rng=random.Random(5))
    built = [builder.build(idx) for idx in lists]
    assert built[0][7].tolist() == [7, 100, 2317, 101] and tuple(built[0][1].shape) == (4, 25, 1)
    assert not bool((built[0][2][:, :5, 2:] <= 0).any())
    for step, batch in enumerate(built):
        G, D = trainer.step(batch)
        for k, val in list(G.items()) + list(D.items()):
            assert bool(torch.isfinite(val).all()), "step %d: %s" % (step, k)
    builder.close()
    ahead = folder_builder(ds, opt, trainer, cuda, rng=random.Random(5))
    for want, got in zip(built, ahead.batches(lists)):
        torch.cuda.synchronize()
        assert all((a is None and b is None) or torch.equal(a, b) for a, b in zip(want, got))
    assert ahead.steps == 2 and 0 <= ahead.waited <= 2
    ahead.close()
    # the default stream of a builder is its own, seeded from the rank: two builders draw alike, and not from `random`
    state = random.getstate()
    one, two = (folder_builder(ds, opt, trainer, cuda) for _ in range(2))
    assert one.rng is not two.rng and one.rng.random() == two.rng.random() and random.getstate() == state
    one.close()
    two.close()


# ------------------------------------------------------------------------------------------------- 3. command lines
def test_command_lines_train_and_validate_on_the_folder(cuda, folder, tmp_path, capsys):
    from canonicalsg2im_amd.scripts import evaluate as val_cli, train as train_cli
    root, base = folder[:2]
    out = str(tmp_path / "out")
    common = [a for a in MODEL] + ["--dataroot", root]
    train_cli.main(common + ["--num_iterations", "2", "--print_every", "1", "--output_dir", out, "--checkpoint_every", "2"])
    lines = capsys.readouterr().out.splitlines()
    data = [k for k, l in enumerate(lines) if l == "data: 4 pictures of %s, 2 loader threads" % os.path.join(base, "images")]
    loader = [k for k, l in enumerate(lines) if l.startswith("loader: ") and l.endswith("of 2 steps waited for their batch")]
    assert len(data) == 1 and len(loader) == 1 and data[0] < loader[0], lines
    assert sum(l.startswith("t = ") for l in lines) == 2
    assert MODEL[-2:] == ["--min_objects", "1"]                          # the synthetic batches keep their own object range
    train_cli.main(MODEL[:-2] + ["--dataroot", str(tmp_path / "nowhere"), "--num_iterations", "1", "--print_every", "1"])
    lines = capsys.readouterr().out.splitlines()
    assert "data: seeded synthetic batches (packed_vg shapes)" in lines and not any(l.startswith("loader:") for l in lines)
    ck = os.path.join(out, "itr_2.pt")
    val_cli.main(common + ["--checkpoint_name", ck, "--num_val_samples", "4"])
    lines = capsys.readouterr().out.splitlines()
    assert "data: 4 pictures of %s" % os.path.join(base, "images") in lines
    val = [l for l in lines if l.startswith("Iter: 2, ")]
    assert len(val) == 2 and "GT VAL avg_iou:" in val[0] and val[1].startswith("Iter: 2, VAL avg_iou:"), lines
    other = str(tmp_path / "other")
    vc.write_folder(other, split="val", extra_predicate=True)
    with pytest.raises(SystemExit, match="the val split's predicates .47 names. are not the model's .46 names."):
        val_cli.main([a for a in MODEL] + ["--dataroot", other, "--checkpoint_name", ck, "--num_val_samples", "4"])
